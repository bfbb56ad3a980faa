// The region graph and its merge loops: mean / histogram-quantile agglomeration (agg_*) and the blockwise RAG edge scoring
// (rag_*), which share the graph build (agg_edges_kernel) and the workspace (AggWs, seg_internal.h).
#include <new>

#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {
// agglo_host.cpp: the merge loop of the histogram-quantile scorers
void host_agglomerate_hist(uint32_t nn, uint32_t ne, const uint32_t* eu, const uint32_t* ev, uint32_t* hist, int quantile,
                           int init_with_max, const float* thresholds, int nthr, uint32_t* roots_out);

// ------------------------------------------------------------------------------------------
// agglomeration
// ------------------------------------------------------------------------------------------
constexpr int AGG_LDS_HEAP = 12288;  // entries (8 B) of the merge queue kept in LDS

__global__ void agg_maxid_kernel(const uint64_t* __restrict__ frags, size_t n, AggWs w) {
  unsigned long long m = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    m = frags[i] > m ? frags[i] : m;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_down(m, o);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax((unsigned long long*)w.maxid, m);
}

__global__ void agg_mark_kernel(const uint64_t* __restrict__ frags, size_t n, AggWs w) {
  const uint64_t maxid = *w.maxid;
  if (maxid >= w.id_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&w.counters[3], 1u);
    return;
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[i];
    if (f) w.rank_of_id[f] = 1u;  // benign race: every writer stores 1
  }
}

// single workgroup: exclusive scan of the presence flags -> ranks (ascending id = sorted order)
__global__ __launch_bounds__(1024) void agg_rank_kernel(AggWs w) {
  __shared__ uint32_t sh[1024];
  if (w.counters[3]) return;
  const uint64_t maxid = *w.maxid;
  const uint32_t n = (uint32_t)maxid + 1;
  const uint32_t chunk = (n + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * chunk, c1 = min(n, c0 + chunk);
  uint32_t cnt = 0;
  for (uint32_t i = c0; i < c1 && i < n; ++i) cnt += w.rank_of_id[i] == 1u;
  sh[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0;
    for (int t = 0; t < 1024; ++t) { const uint32_t c = sh[t]; sh[t] = acc; acc += c; }
    w.counters[0] = acc;
    if (acc > w.node_cap) atomicOr(&w.counters[3], 2u);
  }
  __syncthreads();
  if (w.counters[3]) return;
  uint32_t r = sh[threadIdx.x];
  for (uint32_t i = c0; i < c1 && i < n; ++i) {
    if (w.rank_of_id[i] == 1u) {
      w.rank_of_id[i] = r;
      w.ids[r] = i;
      w.head[r] = NOEDGE;
      w.parent[r] = r;
      ++r;
    } else {
      w.rank_of_id[i] = 0xffffffffu;
    }
  }
}

template <bool HASH>
__device__ __forceinline__ uint32_t agg_rank(const AggWs& w, uint64_t f) {
  if constexpr (!HASH) return w.rank_of_id[f];
  uint32_t s = (uint32_t)mix64(f) & (w.icap - 1);
  for (uint32_t probe = 0; probe < w.icap; ++probe) {
    const uint64_t k = w.idkeys[s];
    if (k == f) return w.idvals[s];
    if (k == HEMPTY) break;
    s = (s + 1) & (w.icap - 1);
  }
  return 0;  // unreachable: every voxel id was inserted by rag_ids_kernel
}

template <bool HASH>
__device__ __forceinline__ void agg_edges_body(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, int D, int H,
                                 int W, const AggWs& w) {
  if (w.counters[3]) return;
  const size_t n = (size_t)D * H * W;
  const size_t hw = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f1 = frags[p];
    if (!f1) continue;
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const int z = (int)(p / hw);
    const uint32_t r1 = agg_rank<HASH>(w, f1);
    const bool ok[3] = {z > 0, y > 0, x > 0};
    const size_t st[3] = {hw, (size_t)W, 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!ok[d]) continue;
      const uint64_t f2 = frags[p - st[d]];
      if (!f2 || f2 == f1) continue;
      const uint32_t r2 = agg_rank<HASH>(w, f2);
      const uint32_t u = r1 < r2 ? r1 : r2, v = r1 < r2 ? r2 : r1;
      const uint64_t key = ((uint64_t)u << 32) | v;
      uint32_t slot = (uint32_t)mix64(key) & (w.hcap - 1);
      bool placed = false;
      for (uint32_t probe = 0; probe < w.hcap; ++probe) {
        const unsigned long long old = atomicCAS((unsigned long long*)&w.hkeys[slot], HEMPTY, key);
        if (old == HEMPTY || old == key) { placed = true; break; }
        slot = (slot + 1) & (w.hcap - 1);
      }
      if (!placed) { atomicOr(&w.counters[3], 4u); return; }
      atomicAdd(&w.hsum[slot], (unsigned long long)affs[(size_t)d * n + p]);
      atomicAdd(&w.hcnt[slot], 1u);
    }
  }
}
template <bool HASH>
__global__ void agg_edges_kernel(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, int D, int H,
                                 int W, AggWs w) {
  agg_edges_body<HASH>(affs, frags, D, H, W, w);
}
__global__ void agg_edges_batch_kernel(const BatchBlock* __restrict__ tab, int D, int H, int W) {
  const BatchBlock& b = tab[blockIdx.y];
  agg_edges_body<true>(b.g.affs, b.g.frags, D, H, W, b.agg);
}

__global__ void agg_compact_kernel(AggWs w) {
  if (w.counters[3]) return;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < w.hcap; s += gridDim.x * blockDim.x) {
    const uint64_t key = w.hkeys[s];
    if (key == HEMPTY) continue;
    const uint32_t e = atomicAdd(&w.counters[1], 1u);
    if (e >= w.edge_cap) { atomicOr(&w.counters[3], 8u); continue; }
    const uint32_t u = (uint32_t)(key >> 32), v = (uint32_t)key;
    w.eu[e] = u; w.ev[e] = v; w.ekey0[e] = key;
    w.esum[e] = w.hsum[s]; w.ecnt[e] = w.hcnt[s];
    w.eflags[e] = 0;
    w.hvals[s] = e;
    w.enextu[e] = atomicExch(&w.head[u], e);
    w.enextv[e] = atomicExch(&w.head[v], e);
  }
}

// Histogram-quantile scorers (reference post/watershed.py:230-243): the 256-bin histogram of every edge's affinities, in a
// second scan once the edges are numbered (hist [ne][256]; the merge loop of these scorers runs on the host, agglo_host.cpp).
__global__ void agg_hist_kernel(const uint8_t* __restrict__ affs, const uint64_t* __restrict__ frags, int D, int H, int W, AggWs w,
                                uint32_t* __restrict__ hist) {
  if (w.counters[3]) return;
  const size_t n = (size_t)D * H * W;
  const size_t hw = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f1 = frags[p];
    if (!f1) continue;
    const int x = (int)(p % W);
    const int y = (int)((p / W) % H);
    const int z = (int)(p / hw);
    const uint32_t r1 = w.rank_of_id[f1];
    const bool ok[3] = {z > 0, y > 0, x > 0};
    const size_t st[3] = {hw, (size_t)W, 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!ok[d]) continue;
      const uint64_t f2 = frags[p - st[d]];
      if (!f2 || f2 == f1) continue;
      const uint32_t r2 = w.rank_of_id[f2];
      const uint32_t u = r1 < r2 ? r1 : r2, v = r1 < r2 ? r2 : r1;
      const uint64_t key = ((uint64_t)u << 32) | v;
      uint32_t slot = (uint32_t)mix64(key) & (w.hcap - 1);
      while (w.hkeys[slot] != key) slot = (slot + 1) & (w.hcap - 1);  // present: agg_edges_kernel inserted every pair
      atomicAdd(&hist[(size_t)w.hvals[slot] * 256 + affs[(size_t)d * n + p]], 1u);
    }
  }
}

// Ties of the merge queue are broken by the edge's initial key (oracle/seg_ref.c).  The mean affinities of uint8 sums tie
// often, and looking the two keys up costs the single-lane loop two trips to L2 per comparison: 3.3 us per pop.  So the
// edges are ranked by their key once, here (one workgroup, keys in LDS, rank = number of smaller keys), and the queue
// entries carry the rank: a comparison is then one 64-bit compare.  Graphs of more than kRankMax edges keep the look-up.
// erank = w.qnext (an array the mean-agglomeration path does not use otherwise); counters[7] = ranks valid.
constexpr uint32_t kRankMax = AGG_LDS_HEAP;  // ranked <=> the merge loop's FAST form (queue, flags and ranks fit the LDS)
__global__ __launch_bounds__(1024) void agg_edge_rank_kernel(AggWs w) {
  extern __shared__ uint64_t rank_keys[];
  if (w.counters[3]) return;
  const uint32_t ne = w.counters[1];
  if (ne > kRankMax || ne > w.edge_cap) return;
  for (uint32_t e = threadIdx.x; e < ne; e += blockDim.x) rank_keys[e] = w.ekey0[e];
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < ne; e += blockDim.x) {
    const uint64_t k = rank_keys[e];
    uint32_t r = 0;
    for (uint32_t j = 0; j < ne; ++j) r += rank_keys[j] < k ? 1u : 0u;
    w.qnext[e] = r;
  }
  if (threadIdx.x == 0) w.counters[7] = 1;
}

__device__ __forceinline__ float agg_score(unsigned long long sum, uint32_t cnt) {
  return 1.0f - (float)((double)sum / (255.0 * (double)cnt));
}

// The sequential merge loops hold one CU (its LDS) for tens of milliseconds.  A one-workgroup launch always lands on
// the same XCD, so the eight lanes of the block pipeline would take eight CUs of ONE XCD away from the U-Net's
// persistent conv workgroups (measured with dummy kernels: 8 x 98 KB of LDS held that way cost the predict stream
// 13 %, one CU in each XCD 3 %).  So the loops are launched as 8 workgroups, which the dispatcher deals round-robin
// to the 8 XCDs, and exactly one of them -- the one on the workspace's XCD if there is one, else the last to
// arrive -- does the work; the others leave at once.  claim[0] = taken, claim[1] = arrivals (zero before the launch).
__device__ __forceinline__ bool xcd_claim(uint32_t* claim, int target) {
  __shared__ int sh_run;
  if (threadIdx.x == 0) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    bool run = false;
    if ((int)(xcc & 7) == target) run = atomicCAS(&claim[0], 0u, 1u) == 0u;
    const unsigned arrived = atomicAdd(&claim[1], 1u);
    if (!run && arrived == gridDim.x - 1) run = atomicCAS(&claim[0], 0u, 1u) == 0u;
    sh_run = run ? 1 : 0;
  }
  __syncthreads();
  return sh_run != 0;
}

// One wave per volume; lane 0 replays the sequential merge loop of oracle/seg_ref.c (waterz mergeUntil / mergeRegions:
// on a shared neighbour the dearer of the two parallel edges, by STORED score, is merged into the cheaper one, which
// keeps its place in the queue).  mergeRegions also marks every edge incident to the survivor stale; with this queue --
// a total order on (stored score, initial key) -- rescoring an edge whose sums did not change puts it back exactly
// where it was, so that marking cannot be observed and is not replayed here (the bin queue of rag_merge_kernel, where
// a re-insertion moves the edge to the back of its bin, does replay it).
struct AggThresholds {  // by value: no host-to-device copy per call
  float v[16];
};

// FAST: the graph fits -- ne <= AGG_LDS_HEAP edges, ranked by agg_edge_rank_kernel.  The queue never holds more entries than
// there are edges, so every queue access is a plain LDS access (with the HBM overflow in the same expression the compiler
// selects between the two addresses and emits FLAT loads: 0.25 us per sift level, 3 us per pop); an entry carries
// rank << 16 | edge below the score, so a pop needs no look-up; and the edge flags live in LDS.
template <bool FAST>
__device__ __forceinline__ void agg_merge_body(const AggWs& w, const AggThresholds& thr_arg, int nthr, uint64_t* hl, uint8_t* fl_lds,
                                               int* sh_dummy_p, uint32_t nn, uint32_t ne) {
  const float* thresholds = thr_arg.v;
  int& sh_dummy = *sh_dummy_p;
  if constexpr (FAST) {
    for (uint32_t i = threadIdx.x; i < ne; i += 64) fl_lds[i] = 0;  // agg_compact_kernel left every flag at 0
    __syncthreads();
  }
  auto fget = [&](uint32_t e) -> uint8_t {
    if constexpr (FAST) return fl_lds[e];
    else return w.eflags[e];
  };
  auto fset = [&](uint32_t e, uint8_t v) {
    if constexpr (FAST) fl_lds[e] = v;
    else w.eflags[e] = v;
  };
  const int lane = threadIdx.x;
  int items = 0;  // meaningful on lane 0 only
  const float tmax = thresholds[nthr - 1];
  // entry: [63:32] float bits of the score (scores are >= 0: bit pattern order == value order),
  //        [31:0] edge index; ties on the score are broken by the edge's initial key.
  auto hget = [&](int i) -> uint64_t {
    if constexpr (FAST) return hl[i];
    else return i < AGG_LDS_HEAP ? hl[i] : w.heap_spill[i - AGG_LDS_HEAP];
  };
  auto hset = [&](int i, uint64_t v) {
    if constexpr (FAST) hl[i] = v;
    else { if (i < AGG_LDS_HEAP) hl[i] = v; else w.heap_spill[i - AGG_LDS_HEAP] = v; }
  };
  // low word of an entry: FAST: rank by initial key << 16 | edge; else the edge, and ties look the keys up
  auto less = [&](uint64_t a, uint64_t b) -> bool {
    if constexpr (FAST) return a < b;
    const uint32_t sa = (uint32_t)(a >> 32), sb = (uint32_t)(b >> 32);
    if (sa != sb) return sa < sb;
    return w.ekey0[(uint32_t)a] < w.ekey0[(uint32_t)b];
  };
  auto entry = [&](float sc, uint32_t e) -> uint64_t {
    if constexpr (FAST) return ((uint64_t)__float_as_uint(sc) << 32) | ((uint64_t)w.qnext[e] << 16) | e;
    else return ((uint64_t)__float_as_uint(sc) << 32) | e;
  };
  auto edge_of = [&](uint64_t top) -> uint32_t {
    if constexpr (FAST) return (uint32_t)top & 0xffffu;
    else return (uint32_t)top;
  };
  auto sift_down = [&](int i, uint64_t val) {
    for (;;) {
      const int c1 = 2 * i + 1, c2 = c1 + 1;
      if (c1 >= items) break;
      int sm = c1;
      uint64_t smv = hget(c1);
      if (c2 < items) {
        const uint64_t v2 = hget(c2);
        if (less(v2, smv)) { sm = c2; smv = v2; }
      }
      if (!less(smv, val)) break;
      hset(i, smv);
      i = sm;
    }
    hset(i, val);
  };
  auto push = [&](uint64_t val) {
    int c = items++;
    while (c > 0) {
      const int p = (c - 1) / 2;
      const uint64_t pv = hget(p);
      if (less(val, pv)) { hset(c, pv); c = p; } else break;
    }
    hset(c, val);
  };
  bool fail = false;
  auto hfind = [&](uint64_t key) -> int64_t {
    uint32_t s = (uint32_t)mix64(key) & (w.hcap - 1);
    for (uint32_t probe = 0; probe < w.hcap; ++probe) {
      const uint64_t k = w.hkeys[s];
      if (k == key) return (int64_t)s;
      if (k == HEMPTY) return -1;
      s = (s + 1) & (w.hcap - 1);
    }
    return -1;
  };
  auto hput = [&](uint64_t key, uint32_t val) {
    uint32_t s = (uint32_t)mix64(key) & (w.hcap - 1);
    uint32_t probe = 0;
    for (; probe < w.hcap; ++probe) {
      const uint64_t k = w.hkeys[s];
      if (k == HEMPTY || k == HTOMB || k == key) break;
      s = (s + 1) & (w.hcap - 1);
    }
    if (probe == w.hcap) { fail = true; return; }
    w.hkeys[s] = key;
    w.hvals[s] = val;
  };
  auto norm_key = [](uint32_t x, uint32_t y) -> uint64_t {
    return x < y ? (((uint64_t)x << 32) | y) : (((uint64_t)y << 32) | x);
  };

  if (lane == 0) {
    // initial queue: only edges below the largest threshold can ever be popped
    for (uint32_t e = 0; e < ne; ++e) {
      const float sc = agg_score(w.esum[e], w.ecnt[e]);
      w.escore[e] = sc;
      if (sc < tmax) hset(items++, entry(sc, e));
    }
    for (int i = items / 2 - 1; i >= 0; --i) sift_down(i, hget(i));  // Floyd heapify
  }
  for (int t = 0; t < nthr; ++t) {
    if (lane == 0) {
      const float thr = thresholds[t];
      while (items > 0) {
        const uint64_t top = hget(0);
        if (!(__uint_as_float((uint32_t)(top >> 32)) < thr)) break;
        --items;
        if (items > 0) sift_down(0, hget(items));
        const uint32_t e = edge_of(top);
        const uint8_t fl = fget(e);
        if (fl & 1) continue;
        if (fl & 2) {
          fset(e, fl & ~2);
          const float sc = agg_score(w.esum[e], w.ecnt[e]);
          w.escore[e] = sc;
          if (sc < tmax) push(entry(sc, e));
          continue;
        }
        const uint32_t eu = w.eu[e], evv = w.ev[e];
        const uint32_t a = eu < evv ? eu : evv, b = eu < evv ? evv : eu;
        // Every access below is a dependent trip to L2 (~0.3 us), so the loads that do not depend on each other are
        // issued together: all fields of f at once, the first probes of both hash lookups at once, the sums at once.
        uint32_t f = w.head[b];
        while (f != NOEDGE && !fail) {
          const uint32_t fu = w.eu[f], fv = w.ev[f], fnu = w.enextu[f], fnv = w.enextv[f];
          const uint8_t ffl = fget(f);
          const bool b_in_u = fu == b;
          const uint32_t nxt = b_in_u ? fnu : fnv;
          if (f != e && !(ffl & 1)) {
            const uint32_t nb = b_in_u ? fv : fu;
            const uint64_t fkey = norm_key(fu, fv), gkey = norm_key(a, nb);
            uint32_t sf = (uint32_t)mix64(fkey) & (w.hcap - 1), sg = (uint32_t)mix64(gkey) & (w.hcap - 1);
            uint64_t kf = w.hkeys[sf], kg = w.hkeys[sg];  // both first probes in flight together
            int64_t fs = -1, gs = -1;
            for (uint32_t probe = 0; probe < w.hcap; ++probe) {
              if (kf == fkey) { fs = (int64_t)sf; break; }
              if (kf == HEMPTY) break;
              sf = (sf + 1) & (w.hcap - 1);
              kf = w.hkeys[sf];
            }
            if (fs >= 0) w.hkeys[fs] = HTOMB;
            // (gkey != fkey: a tombstone at fs and the key it replaces both mean "keep probing" to the lookup of gkey)
            for (uint32_t probe = 0; probe < w.hcap; ++probe) {
              if (kg == gkey) { gs = (int64_t)sg; break; }
              if (kg == HEMPTY) break;
              sg = (sg + 1) & (w.hcap - 1);
              kg = sg == (uint32_t)fs ? HTOMB : w.hkeys[sg];
            }
            bool move_f = true;  // f becomes {a, nb}
            if (gs >= 0) {
              const uint32_t g = w.hvals[gs];
              const unsigned long long sum_f = w.esum[f], sum_g = w.esum[g];
              const uint32_t cnt_f = w.ecnt[f], cnt_g = w.ecnt[g];
              const float st_f = w.escore[f], st_g = w.escore[g];
              const uint8_t gfl = fget(g);
              if (st_f > st_g) {  // the a-side edge is the cheaper one: it takes f's sums and keeps its place
                w.esum[g] = sum_g + sum_f;
                w.ecnt[g] = cnt_g + cnt_f;
                fset(g, gfl | 2);
                fset(f, ffl | 1);
                move_f = false;
              } else {            // f is the cheaper one (or ties): it takes g's sums and g's slot in the edge table
                w.esum[f] = sum_f + sum_g;
                w.ecnt[f] = cnt_f + cnt_g;
                fset(g, gfl | 1);
                w.hvals[gs] = f;
              }
            }
            if (move_f) {
              // b is replaced IN ITS SLOT so that nb's list keeps following the link that belongs to nb's slot;
              // f joins a's list through b's old slot
              const uint32_t ha = w.head[a];
              if (b_in_u) { w.eu[f] = a; w.enextu[f] = ha; } else { w.ev[f] = a; w.enextv[f] = ha; }
              w.head[a] = f;
              fset(f, ffl | 2);
              if (gs < 0) hput(gkey, f);
            }
          }
          f = nxt;
        }
        if (fail) break;
        {
          const int64_t es = hfind(norm_key(eu, evv));
          if (es >= 0) w.hkeys[es] = HTOMB;
        }
        fset(e, fget(e) | 1);
        w.parent[b] = a;
      }
      sh_dummy = items;
      if (fail) atomicOr(&w.counters[3], 16u);
    }
    __syncthreads();
    // snapshot of the roots at this threshold (parents always point to smaller ranks)
    for (uint32_t i = lane; i < nn; i += 64) {
      uint32_t r = i;
      for (;;) {
        const uint32_t p = __hip_atomic_load(&w.parent[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == r) break;
        r = p;
      }
      w.roots[(size_t)t * w.node_cap + i] = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void agg_merge_kernel(AggWs w, const AggThresholds thr_arg, int nthr) {
  __shared__ uint64_t hl[AGG_LDS_HEAP];
  __shared__ uint8_t fl_lds[AGG_LDS_HEAP];
  __shared__ int sh_dummy;
  static_assert(AGG_LDS_HEAP <= 65536, "FAST entries hold 16-bit ranks and edges");
  if (!xcd_claim(&w.counters[5], w.xcd_hint)) return;
  if (w.counters[3]) return;
  const uint32_t nn = w.counters[0];
  const uint32_t ne = min(w.counters[1], w.edge_cap);
  if (ne <= (uint32_t)AGG_LDS_HEAP && w.counters[7] != 0) agg_merge_body<true>(w, thr_arg, nthr, hl, fl_lds, &sh_dummy, nn, ne);
  else agg_merge_body<false>(w, thr_arg, nthr, hl, fl_lds, &sh_dummy, nn, ne);
}

__global__ void agg_relabel_kernel(const uint64_t* __restrict__ frags, size_t n, int nthr, AggWs w,
                                   uint64_t* __restrict__ segs) {
  keep_overflow(w);
  if (w.counters[3]) return;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[p];
    if (!f) {
      for (int t = 0; t < nthr; ++t) segs[(size_t)t * n + p] = 0;
      continue;
    }
    const uint32_t r = w.rank_of_id[f];
    for (int t = 0; t < nthr; ++t) segs[(size_t)t * n + p] = w.ids[w.roots[(size_t)t * w.node_cap + r]];
  }
}

// ------------------------------------------------------------------------------------------
// per-block RAG edge scoring (reference post/blockwise/waterz_agglom.py:106-170); restated in
// oracle/seg_ref.c seg_rag_merge_scores_u8
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void rag_ids_body(const uint64_t* __restrict__ frags, size_t n, int W, const AggWs& w) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[p];
    if (!f) continue;
    if (p % W != 0 && frags[p - 1] == f) continue;  // the run's first voxel inserts the id
    if (f >= HTOMB) { atomicOr(&w.counters[3], 1u); continue; }
    uint32_t s = (uint32_t)mix64(f) & (w.icap - 1);
    bool done = false;
    for (uint32_t probe = 0; probe < w.icap; ++probe) {
      const unsigned long long old = atomicCAS((unsigned long long*)&w.idkeys[s], HEMPTY, f);
      if (old == HEMPTY) {
        const uint32_t i = atomicAdd(&w.counters[0], 1u);
        if (i < w.node_cap) {
          w.idu[i] = f;
          w.idvals[s] = i;  // number in order of insertion (bsmi_rag_graph_u8 works with these; rag_rank_kernel replaces them by ranks)
        } else {
          atomicOr(&w.counters[3], 2u);
        }
        done = true;
        break;
      }
      if (old == f) { done = true; break; }
      s = (s + 1) & (w.icap - 1);
    }
    if (!done) atomicOr(&w.counters[3], 2u);
  }
}
__global__ void rag_ids_kernel(const uint64_t* __restrict__ frags, size_t n, int W, AggWs w) { rag_ids_body(frags, n, W, w); }
__global__ void rag_ids_batch_kernel(const BatchBlock* __restrict__ tab, size_t n, int W) {
  const BatchBlock& b = tab[blockIdx.y];
  rag_ids_body(b.g.frags, n, W, b.agg);
}

__global__ void rag_pad_kernel(AggWs w) {
  const uint32_t nn = min(w.counters[0], w.node_cap);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < w.node_cap; i += gridDim.x * blockDim.x)
    if (i >= nn) w.idu[i] = HEMPTY;
}

__global__ void rag_rank_kernel(AggWs w) {
  if (w.counters[3]) return;
  const uint32_t nn = w.counters[0];
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nn; r += gridDim.x * blockDim.x) {
    const uint64_t f = w.ids[r];
    uint32_t s = (uint32_t)mix64(f) & (w.icap - 1);
    while (w.idkeys[s] != f) s = (s + 1) & (w.icap - 1);
    w.idvals[s] = r;
    w.head[r] = NOEDGE;
    w.parent[r] = r;
    w.cur[r] = r;
    w.tnext[r] = NOEDGE;
    w.ntime[r] = 0;
  }
}

__global__ void rag_iota_kernel(AggWs w) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < w.hcap; i += gridDim.x * blockDim.x) w.iota[i] = i;
}

// edges numbered in ascending (u, v) order: edge e = position of its key in the sorted table
__global__ void rag_compact_kernel(AggWs w) {
  if (w.counters[3]) return;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < w.hcap; i += gridDim.x * blockDim.x) {
    const uint64_t key = w.skeys[i];
    if (key == HEMPTY) continue;
    if (i >= w.edge_cap) { atomicOr(&w.counters[3], 8u); continue; }
    const uint32_t e = i, slot = w.sslot[i];
    const uint32_t u = (uint32_t)(key >> 32), v = (uint32_t)key;
    w.eu[e] = u; w.ev[e] = v; w.ekey0[e] = key;
    w.esum[e] = w.hsum[slot]; w.ecnt[e] = w.hcnt[slot];
    w.eflags[e] = 0;
    w.hvals[slot] = e;
    w.enextu[e] = atomicExch(&w.head[u], e);
    w.enextv[e] = atomicExch(&w.head[v], e);
    atomicMax(&w.counters[1], i + 1);
  }
}

__device__ __forceinline__ int64_t agg_hfind(const AggWs& w, uint64_t key) {
  uint32_t s = (uint32_t)mix64(key) & (w.hcap - 1);
  for (uint32_t probe = 0; probe < w.hcap; ++probe) {
    const uint64_t k = w.hkeys[s];
    if (k == key) return (int64_t)s;
    if (k == HEMPTY) return -1;
    s = (s + 1) & (w.hcap - 1);
  }
  return -1;
}

__device__ __forceinline__ bool agg_hput(const AggWs& w, uint64_t key, uint32_t val) {
  uint32_t s = (uint32_t)mix64(key) & (w.hcap - 1);
  uint32_t probe = 0;
  for (; probe < w.hcap; ++probe) {
    const uint64_t k = w.hkeys[s];
    if (k == HEMPTY || k == HTOMB || k == key) break;
    s = (s + 1) & (w.hcap - 1);
  }
  if (probe == w.hcap) return false;
  w.hkeys[s] = key;
  w.hvals[s] = val;
  return true;
}

__device__ __forceinline__ uint64_t agg_norm_key(uint32_t x, uint32_t y) {
  return x < y ? (((uint64_t)x << 32) | y) : (((uint64_t)y << 32) | x);
}

// ---- RAG path: bin-queue merge loop ---------------------------------------------------------------------------------
// Where the loop's per-edge state lives.  FAST (ne <= kRagFastEdges, nn <= kRagFastNodes: every 160^3 read box so far):
// endpoints, queue links, merge clocks, flags (16-bit / 8-bit), affinity sums, counts and stored scores (32-bit) as LDS
// arrays, 138 KB, so that a pop -- and most pops only find a stale edge to re-score: every merge makes all edges at the
// survivor stale, ten or more re-scorings per merge -- touches no HBM at all.  Otherwise the arrays of the workspace.
constexpr int kRagFastEdges = 6144, kRagFastNodes = 6144;
template <bool FAST>
struct RagMem {
  const AggWs& w;
  uint16_t *eu16, *ev16, *qn16, *et16, *nt16;
  uint8_t* fl8;
  uint32_t *sum32, *cnt32;  // a sum of affinity bytes over at most 3 * 160^3 voxel faces fits 32 bits
  float* sc32;
  __device__ __forceinline__ unsigned long long sum(uint32_t e) const { if constexpr (FAST) return sum32[e]; else return w.esum[e]; }
  __device__ __forceinline__ uint32_t cnt(uint32_t e) const { if constexpr (FAST) return cnt32[e]; else return w.ecnt[e]; }
  __device__ __forceinline__ void fold(uint32_t into, uint32_t from) const {   // the sums of `from` join those of `into`
    if constexpr (FAST) { sum32[into] += sum32[from]; cnt32[into] += cnt32[from]; }
    else { w.esum[into] += w.esum[from]; w.ecnt[into] += w.ecnt[from]; }
  }
  __device__ __forceinline__ float score(uint32_t e) const { if constexpr (FAST) return sc32[e]; else return w.escore[e]; }
  __device__ __forceinline__ void set_score(uint32_t e, float v) const { if constexpr (FAST) sc32[e] = v; else w.escore[e] = v; }
  __device__ __forceinline__ uint32_t eu(uint32_t e) const { if constexpr (FAST) return eu16[e]; else return w.eu[e]; }
  __device__ __forceinline__ uint32_t ev(uint32_t e) const { if constexpr (FAST) return ev16[e]; else return w.ev[e]; }
  __device__ __forceinline__ void set_eu(uint32_t e, uint32_t v) const { if constexpr (FAST) eu16[e] = (uint16_t)v; else w.eu[e] = v; }
  __device__ __forceinline__ void set_ev(uint32_t e, uint32_t v) const { if constexpr (FAST) ev16[e] = (uint16_t)v; else w.ev[e] = v; }
  __device__ __forceinline__ bool dead(uint32_t e) const { if constexpr (FAST) return fl8[e] & 1; else return w.eflags[e] & 1; }
  __device__ __forceinline__ void kill(uint32_t e) const { if constexpr (FAST) fl8[e] |= 1; else w.eflags[e] |= 1; }
  __device__ __forceinline__ uint32_t qnext(uint32_t e) const {
    if constexpr (FAST) { const uint16_t v = qn16[e]; return v == 0xffffu ? NOEDGE : (uint32_t)v; }
    else return w.qnext[e];
  }
  __device__ __forceinline__ void set_qnext(uint32_t e, uint32_t v) const { if constexpr (FAST) qn16[e] = (uint16_t)v; else w.qnext[e] = v; }
  __device__ __forceinline__ uint32_t etime(uint32_t e) const { if constexpr (FAST) return et16[e]; else return w.etime[e]; }
  __device__ __forceinline__ void set_etime(uint32_t e, uint32_t v) const { if constexpr (FAST) et16[e] = (uint16_t)v; else w.etime[e] = v; }
  __device__ __forceinline__ uint32_t ntime(uint32_t n) const { if constexpr (FAST) return nt16[n]; else return w.ntime[n]; }
  __device__ __forceinline__ void set_ntime(uint32_t n, uint32_t v) const { if constexpr (FAST) nt16[n] = (uint16_t)v; else w.ntime[n] = v; }
};

// contract live edge e: b = larger endpoint is absorbed by a (same rewiring as agg_merge_kernel).  Staleness in this path
// is a clock comparison (rag_merge_body), so nothing is flagged here: every edge that ends up incident to a is stale
// because a's clock moves.  Sequential form (one lane).
template <bool FAST>
__device__ __forceinline__ bool agg_contract(const RagMem<FAST>& M, uint32_t e) {
  const AggWs& w = M.w;
  const uint32_t eu = M.eu(e), evv = M.ev(e);
  const uint32_t a = eu < evv ? eu : evv, b = eu < evv ? evv : eu;
  uint32_t f = w.head[b];
  while (f != NOEDGE) {
    const uint32_t fu = M.eu(f), fv = M.ev(f);
    const bool b_in_u = fu == b;
    const uint32_t nxt = b_in_u ? w.enextu[f] : w.enextv[f];
    if (f != e && !M.dead(f)) {
      const uint32_t nb = b_in_u ? fv : fu;
      const uint64_t gkey = agg_norm_key(a, nb);
      const int64_t fs = agg_hfind(w, agg_norm_key(fu, fv));
      if (fs >= 0) w.hkeys[fs] = HTOMB;
      const int64_t gs = agg_hfind(w, gkey);
      bool move_f = true;
      if (gs >= 0) {
        const uint32_t g = w.hvals[gs];
        if (M.score(f) > M.score(g)) {
          M.fold(g, f);
          M.kill(f);
          move_f = false;
        } else {
          M.fold(f, g);
          M.kill(g);
          w.hvals[gs] = f;
        }
      }
      if (move_f) {
        if (b_in_u) { M.set_eu(f, a); w.enextu[f] = w.head[a]; } else { M.set_ev(f, a); w.enextv[f] = w.head[a]; }
        w.head[a] = f;
        if (gs < 0 && !agg_hput(w, gkey, f)) return false;
      }
    }
    f = nxt;
  }
  const int64_t es = agg_hfind(w, agg_norm_key(eu, evv));
  if (es >= 0) w.hkeys[es] = HTOMB;
  M.kill(e);
  w.parent[b] = a;
  return true;
}

constexpr int kMaxQueueBins = 1024;
constexpr int kSweepCap = 2048;  // incident edges the cooperative sweep takes per contraction (more: lane 0 alone, agg_contract)

// agg_contract by the whole wave (all 64 lanes call it with the same e, after a __syncthreads()).  The edges at b are
// independent of one another -- each meets a different neighbour -- so lane 0 only walks b's list into LDS (one memory
// round trip per edge) and the lanes then take one incident edge each: the two hash look-ups, the comparison of the stored
// scores, the fold or the move.  What must keep the order of the sequential loop does: the moved edges are linked into a's
// list in traversal order.  New hash entries go in by compare-and-swap (the slot an entry lands in may differ from the
// sequential run's; look-ups do not care).  -> false: hash table full.
template <bool FAST>
__device__ __forceinline__ bool agg_contract_wave(const RagMem<FAST>& M, uint32_t e, uint32_t* lst, int* sh, uint32_t& a_out, uint32_t& b_out) {
  const AggWs& w = M.w;
  const int lane = threadIdx.x;
  const uint32_t eu = M.eu(e), evv = M.ev(e);
  const uint32_t a = eu < evv ? eu : evv, b = eu < evv ? evv : eu;
  a_out = a;
  b_out = b;
  if (lane == 0) {
    int n = 0;
    uint32_t f = w.head[b];
    while (f != NOEDGE && n < kSweepCap) {
      const uint32_t fu = M.eu(f), nu = w.enextu[f], nv = w.enextv[f];  // independent loads: one round trip per edge
      lst[n++] = f;
      f = fu == b ? nu : nv;
    }
    sh[0] = f == NOEDGE ? n : -1;
  }
  __syncthreads();
  const int n = sh[0];
  if (n < 0) {  // a hub with more edges than the list holds: the sequential form
    if (lane == 0) sh[1] = agg_contract<FAST>(M, e) ? 1 : 0;
    __syncthreads();
    return sh[1] != 0;
  }
  uint32_t head_a = w.head[a];
  bool fail = false;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    uint32_t f = NOEDGE;
    bool live = false, b_in_u = false, move_f = false, put_f = false;
    uint64_t gkey = 0;
    if (i < n) {
      f = lst[i];
      live = f != e && !M.dead(f);
    }
    if (live) {
      const uint32_t fu = M.eu(f), fv = M.ev(f);
      b_in_u = fu == b;
      const uint32_t nb = b_in_u ? fv : fu;
      gkey = agg_norm_key(a, nb);
      const int64_t fs = agg_hfind(w, agg_norm_key(fu, fv));
      const int64_t gs = agg_hfind(w, gkey);
      if (fs >= 0) w.hkeys[fs] = HTOMB;
      move_f = true;
      if (gs >= 0) {
        const uint32_t g = w.hvals[gs];
        if (M.score(f) > M.score(g)) {
          M.fold(g, f);
          M.kill(f);
          move_f = false;
        } else {
          M.fold(f, g);
          M.kill(g);
          w.hvals[gs] = f;
        }
      } else {
        put_f = true;
      }
    }
    // link the moved edges into a's list in traversal order: each one in front of the previous mover
    const unsigned long long movers = __ballot(move_f);
    const unsigned long long lower = movers & ((1ull << lane) - 1ull);
    const int prev_lane = lower ? 63 - __builtin_clzll(lower) : lane;
    const uint32_t prev_f = __shfl(f, prev_lane);  // every lane takes part
    if (move_f) {
      const uint32_t link = lower ? prev_f : head_a;
      if (b_in_u) { M.set_eu(f, a); w.enextu[f] = link; } else { M.set_ev(f, a); w.enextv[f] = link; }
    }
    if (movers) head_a = __shfl(f, 63 - __builtin_clzll(movers));
    // new entries (a, nb) -> f
    if (put_f) {
      uint32_t s = (uint32_t)mix64(gkey) & (w.hcap - 1);
      bool placed = false;
      for (uint32_t probe = 0; probe < 2 * w.hcap && !placed; ++probe) {
        const unsigned long long k = ((volatile unsigned long long*)w.hkeys)[s];
        if (k == HEMPTY || k == HTOMB) {
          if (atomicCAS((unsigned long long*)&w.hkeys[s], k, (unsigned long long)gkey) == k) {
            w.hvals[s] = f;
            placed = true;
          }
          continue;  // lost the slot to another lane this instant: look at it again (it holds that lane's key now)
        }
        s = (s + 1) & (w.hcap - 1);
      }
      if (!placed) fail = true;
    }
    __syncthreads();  // the next chunk's look-ups see this chunk's table
  }
  if (lane == 0) {
    w.head[a] = head_a;
    const int64_t es = agg_hfind(w, agg_norm_key(eu, evv));
    if (es >= 0) w.hkeys[es] = HTOMB;
    M.kill(e);
    w.parent[b] = a;
  }
  const bool any_fail = __any(fail);
  __syncthreads();  // the sweep's stores are in place before lane 0 goes on
  return !any_fail;
}

// One wave replays the sequential bin-queue merge loop and grows the merge tree: lane 0 owns the queue and the
// decisions, the contraction of a popped edge is shared by the lanes (agg_contract_wave).
template <bool FAST>
__device__ __forceinline__ void rag_merge_body(const RagMem<FAST>& M, float threshold, int nbins, uint32_t nn, uint32_t ne, uint32_t* bhead,
                                               uint32_t* btail, uint32_t* lst, int* sh) {
  const AggWs& w = M.w;
  const int lane = threadIdx.x;
  int minbin = nbins;            // lane 0's
  const float scale = (float)(nbins - 1);
  auto push = [&](uint32_t e, float sc) {
    int b = (int)(sc * scale);
    b = b < 0 ? 0 : (b > nbins - 1 ? nbins - 1 : b);
    M.set_qnext(e, NOEDGE);
    if (bhead[b] == NOEDGE) bhead[b] = e; else M.set_qnext(btail[b], e);
    btail[b] = e;
    if (b < minbin) minbin = b;
  };
  // initial state and scores by all lanes, the pushes (edge order) by lane 0
  for (uint32_t e = lane; e < ne; e += 64) {
    if constexpr (FAST) {
      M.set_eu(e, w.eu[e]);
      M.set_ev(e, w.ev[e]);
      M.fl8[e] = 0;  // rag_compact_kernel left every flag at 0
      M.sum32[e] = (uint32_t)w.esum[e];
      M.cnt32[e] = w.ecnt[e];
    }
    M.set_score(e, agg_score(M.sum(e), M.cnt(e)));
    M.set_etime(e, 0);
  }
  if constexpr (FAST)
    for (uint32_t n = lane; n < nn; n += 64) M.set_ntime(n, 0);  // as rag_rank_kernel left the workspace's
  __syncthreads();
  if (lane == 0)
    for (uint32_t e = 0; e < ne; ++e) {
      const float sc = M.score(e);
      if (sc < threshold) push(e, sc);
    }
  // mergeRegions marks every edge incident to the survivor stale -- its own, the moved and the merged ones alike.
  // That is a clock: a merge stamps its survivor (ntime), scoring stamps the edge (etime), and an edge is stale when
  // one of its endpoints was stamped after it.
  uint32_t nm = 0, clock = 0;    // lane 0's
  for (;;) {
    // lane 0: pop until an edge is due for a merge (sh[2] = the edge, NOEDGE: queue empty)
    if (lane == 0) {
      uint32_t pick = NOEDGE;
      for (;;) {
        while (minbin < nbins && bhead[minbin] == NOEDGE) ++minbin;
        if (minbin >= nbins) break;
        const uint32_t e = bhead[minbin];
        bhead[minbin] = M.qnext(e);
        if (M.dead(e)) continue;
        const uint32_t tu = M.ntime(M.eu(e)), tv = M.ntime(M.ev(e));
        if (M.etime(e) < (tu > tv ? tu : tv)) {
          const float sc = agg_score(M.sum(e), M.cnt(e));
          M.set_score(e, sc);
          M.set_etime(e, clock);
          if (sc < threshold) push(e, sc);
          continue;
        }
        pick = e;
        break;
      }
      sh[2] = (int)pick;
    }
    __syncthreads();
    const uint32_t e = (uint32_t)sh[2];
    if (e == NOEDGE) break;
    uint32_t a, b;
    if (!agg_contract_wave<FAST>(M, e, lst, sh, a, b)) {
      if (lane == 0) atomicOr(&w.counters[3], 16u);
      break;
    }
    if (lane == 0) {
      const float sc = M.score(e);
      M.set_ntime(a, ++clock);
      const uint32_t t = nn + nm;
      w.tnext[w.cur[a]] = t;
      w.tnext[w.cur[b]] = t;
      w.cur[a] = t;
      w.tnext[t] = NOEDGE;
      w.tscore[t] = sc;
      w.ha[nm] = a;
      w.hb[nm] = b;
      ++nm;
    }
  }
  if (lane == 0) w.counters[4] = nm;
}

__global__ __launch_bounds__(64) void rag_merge_kernel(AggWs w, float threshold, int nbins, int allow_fast) {
  __shared__ uint32_t bhead[kMaxQueueBins], btail[kMaxQueueBins];
  __shared__ uint32_t lst[kSweepCap];
  __shared__ int sh[4];
  __shared__ uint16_t l_eu[kRagFastEdges], l_ev[kRagFastEdges], l_qn[kRagFastEdges], l_et[kRagFastEdges], l_nt[kRagFastNodes];
  __shared__ uint8_t l_fl[kRagFastEdges];
  __shared__ uint32_t l_sum[kRagFastEdges], l_cnt[kRagFastEdges];
  __shared__ float l_sc[kRagFastEdges];
  if (!xcd_claim(&w.counters[5], w.xcd_hint)) return;
  if (w.counters[3]) return;
  for (int b = threadIdx.x; b < nbins; b += 64) bhead[b] = btail[b] = NOEDGE;
  __syncthreads();
  const uint32_t nn = w.counters[0];
  const uint32_t ne = min(w.counters[1], w.edge_cap);
  if (allow_fast && ne <= (uint32_t)kRagFastEdges && nn <= (uint32_t)kRagFastNodes) {
    const RagMem<true> M{w, l_eu, l_ev, l_qn, l_et, l_nt, l_fl, l_sum, l_cnt, l_sc};
    rag_merge_body<true>(M, threshold, nbins, nn, ne, bhead, btail, lst, sh);
  } else {
    const RagMem<false> M{w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    rag_merge_body<false>(M, threshold, nbins, nn, ne, bhead, btail, lst, sh);
  }
}

// score of RAG edge {u, v} = score of the lowest common ancestor in the merge tree (tree nodes
// are numbered in creation order, so the smaller index is always the one to climb)
__global__ void rag_scores_kernel(AggWs w, uint64_t* __restrict__ edges, float* __restrict__ scores, uint64_t cap,
                                  uint64_t* __restrict__ merges, float* __restrict__ mscores, uint64_t* __restrict__ counts) {
  keep_overflow(w);
  if (w.counters[3]) return;
  const uint32_t nn = w.counters[0];
  const uint32_t ne = min(w.counters[1], w.edge_cap);
  const uint32_t nm = w.counters[4];
  if (ne > cap) {  // the caller's edge buffer is too small: say so, and how many entries the block needs (counts[0] > capacity)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicOr(&w.counters[3], 32u);
      atomicOr(w.sticky, 32u);
      counts[0] = ne; counts[1] = nm; counts[2] = nn;
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = ne; counts[1] = nm; counts[2] = nn; }
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += gridDim.x * blockDim.x) {
    const uint64_t key = w.ekey0[e];
    uint32_t x = (uint32_t)(key >> 32), y = (uint32_t)key;
    edges[2 * (size_t)e] = w.ids[x];
    edges[2 * (size_t)e + 1] = w.ids[y];
    float sc = __uint_as_float(0x7fc00000u);
    for (;;) {
      if (x == y) { sc = w.tscore[x]; break; }
      if (x < y) { const uint32_t nx = w.tnext[x]; if (nx == NOEDGE) break; x = nx; }
      else { const uint32_t ny = w.tnext[y]; if (ny == NOEDGE) break; y = ny; }
    }
    scores[e] = sc;
  }
  if (merges)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
      merges[2 * (size_t)i] = w.ids[w.ha[i]];
      merges[2 * (size_t)i + 1] = w.ids[w.hb[i]];
      if (mscores) mscores[i] = w.tscore[nn + i];
    }
}

// The region graph straight out of the edge hash table, for bsmi_rag_graph_u8: nodes carry the numbers rag_ids_kernel gave them
// (insertion order), edges leave in table order; bsmi_rag_merge_scores_host brings them into ascending (id, id) order.  No sort
// on the device: the two radix sorts of the ordered form are 46 of its 60 launches, and a block's task is launch-bound.
__device__ __forceinline__ void rag_graph_hash_out_body(const AggWs& w, uint64_t* __restrict__ edges, uint64_t* __restrict__ sums, uint32_t* __restrict__ cnts,
                                          uint64_t cap, uint64_t* __restrict__ counts) {
  keep_overflow(w);
  if (w.counters[3]) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = w.counters[0];
  for (uint32_t sl = blockIdx.x * blockDim.x + threadIdx.x; sl < w.hcap; sl += gridDim.x * blockDim.x) {
    const uint64_t key = w.hkeys[sl];
    if (key == HEMPTY) continue;
    const unsigned long long e = atomicAdd((unsigned long long*)&counts[0], 1ull);  // (zeroed with the call's tables)
    if (e >= cap) {  // the caller's buffers are too small: say so; counts[0] ends at the number of entries the block needs
      atomicOr(w.sticky, 32u);
      continue;
    }
    const uint64_t a = w.idu[(uint32_t)(key >> 32)], b = w.idu[(uint32_t)key];
    edges[2 * (size_t)e] = a < b ? a : b;
    edges[2 * (size_t)e + 1] = a < b ? b : a;
    sums[e] = w.hsum[sl];
    cnts[e] = w.hcnt[sl];
  }
}
__global__ void rag_graph_hash_out_kernel(AggWs w, uint64_t* __restrict__ edges, uint64_t* __restrict__ sums, uint32_t* __restrict__ cnts,
                                          uint64_t cap, uint64_t* __restrict__ counts) { rag_graph_hash_out_body(w, edges, sums, cnts, cap, counts); }
__global__ void rag_graph_hash_out_batch_kernel(const BatchBlock* __restrict__ tab) {
  const BatchBlock& b = tab[blockIdx.y];
  rag_graph_hash_out_body(b.agg, b.g.edges, b.g.sums, b.g.pair_counts, b.g.edge_capacity, b.g.counts);
}

// fragments -> ids of their merged clusters after rag_merge_kernel, in place (a cluster is named by its smallest id: the
// survivor of every merge is the smaller rank, and ranks ascend with the ids)
__global__ void rag_relabel_kernel(uint64_t* __restrict__ frags, size_t n, AggWs w) {
  keep_overflow(w);
  if (w.counters[3]) return;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint64_t f = frags[p];
    if (!f) continue;
    uint32_t r = agg_rank<true>(w, f);
    for (;;) {
      const uint32_t q = w.parent[r];
      if (q == r) break;
      r = q;
    }
    frags[p] = w.ids[r];
  }
}

// affinity sum and voxel-pair count of every INITIAL edge of the last RAG call, in edge order (the merge loop changes
// esum / ecnt; the hash table rows the edges were compacted from still hold the initial values)
__global__ void rag_edge_stats_kernel(AggWs w, uint64_t* __restrict__ sums, uint64_t* __restrict__ counts, uint64_t cap) {
  if (w.counters[3]) return;
  const uint32_t ne = min(w.counters[1], w.edge_cap);
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < ne && e < cap; e += gridDim.x * blockDim.x) {
    const uint32_t slot = w.sslot[e];
    sums[e] = w.hsum[slot];
    counts[e] = w.hcnt[slot];
  }
}

// clears the per-call tables of the agglomeration (instead of four runtime fill kernels)
__global__ void seg_clear_kernel(AggWs w) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t0; i < w.id_cap; i += stride) w.rank_of_id[i] = 0;
  for (size_t i = t0; i < w.hcap; i += stride) {
    w.hkeys[i] = HEMPTY;
    w.hsum[i] = 0;
    w.hcnt[i] = 0;
  }
}

// bsmi_rag_graph_u8 for rows 0..N-1 of the table (their `fills` launched by the caller); max_hcap: the largest edge table among them
void batch_graph_launch(const BatchBlock* tab, int N, const int64_t shape[3], uint32_t max_hcap, hipStream_t s) {
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  const int bs = 256;
  const dim3 grid((unsigned)std::min<size_t>((n + bs - 1) / bs, 4096), N);
  hipLaunchKernelGGL(rag_ids_batch_kernel, grid, dim3(bs), 0, s, tab, n, (int)shape[2]);
  hipLaunchKernelGGL(agg_edges_batch_kernel, grid, dim3(bs), 0, s, tab, (int)shape[0], (int)shape[1], (int)shape[2]);
  hipLaunchKernelGGL(rag_graph_hash_out_batch_kernel, dim3(std::min<uint32_t>(max_hcap / bs, 2048u), N), dim3(bs), 0, s, tab);
}

int seg_scan_grid() {
  static const int g = [] { const char* e = getenv("BSMI_SEG_SCAN_GRID"); const int v = e ? atoi(e) : 32; return v < 1 ? 1 : v; }();
  return g;
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

// BSMI_AGG_FAST=0 (tests): the general forms of the merge loops (state in the workspace's HBM arrays)
static bool agg_fast_enabled() {
  static const bool fast = [] { const char* e = getenv("BSMI_AGG_FAST"); return !(e && e[0] == '0'); }();
  return fast;
}

int bsmi_agglomerate_mean_u8(bsmi_seg* h, const uint8_t* affs_dev, const uint64_t* frags_dev, const int64_t shape[3],
                             const float* thresholds_host, int n_thresholds, uint64_t* segs_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !thresholds_host || !segs_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_thresholds < 1 || n_thresholds > kMaxThresholds) BSMI_FAIL(BSMI_ERR_INVALID, "1..%d thresholds supported", kMaxThresholds);
  for (int i = 0; i < n_thresholds; ++i) {
    if (!(thresholds_host[i] >= 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "thresholds must be >= 0");
    if (i && thresholds_host[i] < thresholds_host[i - 1]) BSMI_FAIL(BSMI_ERR_INVALID, "thresholds must be ascending");
  }
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  const size_t n = (size_t)D * H * W;
  AggWs& g = h->agg;
  AggThresholds thr;
  static_assert(kMaxThresholds <= 16, "AggThresholds holds 16 values");
  for (int i = 0; i < 16; ++i) thr.v[i] = i < n_thresholds ? thresholds_host[i] : 0.f;
  BSMI_HIP(hipMemsetAsync(g.counters, 0, 8 * sizeof(uint32_t), s));
  BSMI_HIP(hipMemsetAsync(g.maxid, 0, sizeof(uint64_t), s));
  // The scans run as FEW, FAT workgroups (kScanGrid x 1024 threads, grid-stride loops): a lane shares the GPU with
  // the U-Net, whose persistent conv workgroups each need a completely free CU; a 2048-workgroup scan (or a runtime
  // fill kernel) puts a wave on every CU and keeps them all away until it has drained.
  const int bs = 1024;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, (size_t)seg_scan_grid());
  hipLaunchKernelGGL(seg_clear_kernel, dim3(grid), dim3(bs), 0, s, g);
  hipLaunchKernelGGL(agg_maxid_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, g);
  hipLaunchKernelGGL(agg_mark_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, g);
  hipLaunchKernelGGL(agg_rank_kernel, dim3(1), dim3(1024), 0, s, g);
  hipLaunchKernelGGL(agg_edges_kernel<false>, dim3(grid), dim3(bs), 0, s, affs_dev, frags_dev, D, H, W, g);
  hipLaunchKernelGGL(agg_compact_kernel, dim3(grid), dim3(bs), 0, s, g);
  {
    static DeviceOnce once;
    const bool attr_set = once.run([&]() -> int {
      BSMI_HIP(hipFuncSetAttribute((const void*)agg_edge_rank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kRankMax * sizeof(uint64_t))));
      return BSMI_OK;
    }) == BSMI_OK;
    // BSMI_AGG_FAST=0 (tests): leave the edges unranked, i.e. take the general form of the merge loop
    if (attr_set && agg_fast_enabled()) hipLaunchKernelGGL(agg_edge_rank_kernel, dim3(1), dim3(1024), kRankMax * sizeof(uint64_t), s, g);
  }
  hipLaunchKernelGGL(agg_merge_kernel, dim3(8), dim3(64), 0, s, g, thr, n_thresholds);
  hipLaunchKernelGGL(agg_relabel_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, n_thresholds, g, segs_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_agglomerate_hist_u8(bsmi_seg* h, const uint8_t* affs_dev, const uint64_t* frags_dev, const int64_t shape[3],
                             const float* thresholds_host, int n_thresholds, int quantile, int init_with_max, uint64_t* segs_dev,
                             void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !thresholds_host || !segs_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_thresholds < 1 || n_thresholds > kMaxThresholds) BSMI_FAIL(BSMI_ERR_INVALID, "1..%d thresholds supported", kMaxThresholds);
  if (quantile < 0 || quantile > 100) BSMI_FAIL(BSMI_ERR_INVALID, "quantile %d outside 0..100", quantile);
  for (int i = 0; i < n_thresholds; ++i) {
    if (!(thresholds_host[i] >= 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "thresholds must be >= 0");
    if (i && thresholds_host[i] < thresholds_host[i - 1]) BSMI_FAIL(BSMI_ERR_INVALID, "thresholds must be ascending");
  }
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  const size_t n = (size_t)D * H * W;
  AggWs& g = h->agg;
  // region graph on the device, as in bsmi_agglomerate_mean_u8
  BSMI_HIP(hipMemsetAsync(g.counters, 0, 8 * sizeof(uint32_t), s));
  BSMI_HIP(hipMemsetAsync(g.maxid, 0, sizeof(uint64_t), s));
  const int bs = 1024;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, (size_t)seg_scan_grid());
  hipLaunchKernelGGL(seg_clear_kernel, dim3(grid), dim3(bs), 0, s, g);
  hipLaunchKernelGGL(agg_maxid_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, g);
  hipLaunchKernelGGL(agg_mark_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, g);
  hipLaunchKernelGGL(agg_rank_kernel, dim3(1), dim3(1024), 0, s, g);
  hipLaunchKernelGGL(agg_edges_kernel<false>, dim3(grid), dim3(bs), 0, s, affs_dev, frags_dev, D, H, W, g);
  hipLaunchKernelGGL(agg_compact_kernel, dim3(grid), dim3(bs), 0, s, g);
  BSMI_HIP(hipGetLastError());
  uint32_t c[8];
  BSMI_HIP(hipMemcpyAsync(c, g.counters, sizeof c, hipMemcpyDeviceToHost, s));
  BSMI_HIP(hipStreamSynchronize(s));
  if (c[3]) BSMI_FAIL(BSMI_ERR_OVERFLOW, "agglomeration workspace overflow (flags 0x%x: 1 id range, 2 nodes, 4 hash, 8 edges)", c[3]);
  const uint32_t nn = c[0], ne = c[1];
  // per-edge histograms: second scan, then the merge loop on the host (agglo_host.cpp), then the relabel on the device
  // 1 KiB of histogram per edge, on the device and again on the host: say so before a few million edges end in a bare
  // out-of-memory error (this entry point serves the whole-ROI simple_watershed; the block pipeline never builds histograms)
  const size_t hist_bytes = (size_t)ne * 256 * sizeof(uint32_t);
  {
    size_t free_b = 0, total_b = 0;
    BSMI_HIP(hipMemGetInfo(&free_b, &total_b));
    if (hist_bytes > free_b - free_b / 8)
      BSMI_FAIL(BSMI_ERR_OVERFLOW, "histogram-quantile agglomeration of %u edges needs %.1f GB of histograms (1 KiB per edge) on the device and the host, %.1f GB of device memory are free: segment the volume blockwise, or with the mean scorer", ne,
                hist_bytes / 1e9, free_b / 1e9);
  }
  std::vector<uint32_t> eu, ev, hist, roots;
  try {
    eu.resize(ne); ev.resize(ne); hist.resize((size_t)ne * 256); roots.resize((size_t)n_thresholds * std::max(nn, 1u));
  } catch (const std::bad_alloc&) {
    BSMI_FAIL(BSMI_ERR_OVERFLOW, "histogram-quantile agglomeration of %u edges: no %.1f GB of host memory for the histograms", ne, hist_bytes / 1e9);
  }
  if (ne) {
    uint32_t* hist_dev = nullptr;
    BSMI_HIP(hipMalloc((void**)&hist_dev, (size_t)ne * 256 * sizeof(uint32_t)));
    hipError_t err = hipMemsetAsync(hist_dev, 0, (size_t)ne * 256 * sizeof(uint32_t), s);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(agg_hist_kernel, dim3(grid), dim3(bs), 0, s, affs_dev, frags_dev, D, H, W, g, hist_dev);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(hist.data(), hist_dev, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipMemcpyAsync(eu.data(), g.eu, ne * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipMemcpyAsync(ev.data(), g.ev, ne * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    (void)hipFree(hist_dev);
    BSMI_HIP(err);
  }
  host_agglomerate_hist(nn, ne, eu.data(), ev.data(), hist.data(), quantile, init_with_max, thresholds_host, n_thresholds, roots.data());
  for (int t = 0; t < n_thresholds && nn; ++t)
    BSMI_HIP(hipMemcpyAsync(g.roots + (size_t)t * g.node_cap, roots.data() + (size_t)t * nn, nn * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(agg_relabel_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, n_thresholds, g, segs_dev);
  BSMI_HIP(hipGetLastError());
  BSMI_HIP(hipStreamSynchronize(s));  // `roots` (host memory) must outlive the copies
  return BSMI_OK;
}

// ids -> ranks, region graph, bin-queue merge loop up to `threshold` (the common front of the two RAG entry points)
static int rag_build_and_merge(bsmi_seg* h, const uint8_t* affs_dev, const uint64_t* frags_dev, const int64_t shape[3], float threshold,
                               int discretize_queue, uint64_t* counts_dev, hipStream_t s) {
  BSMI_HIP(hipSetDevice(h->device));
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  const int D = (int)shape[0], H = (int)shape[1], W = (int)shape[2];
  AggWs& g = h->agg;
  {
    Fills fl;
    fl.add(g.counters, 8 * sizeof(uint32_t));
    if (counts_dev) fl.add(counts_dev, 3 * sizeof(uint64_t));
    fl.add(g.idkeys, (size_t)g.icap * sizeof(uint64_t), 0xffffffffu);
    fl.add(g.hkeys, (size_t)g.hcap * sizeof(uint64_t), 0xffffffffu);
    fl.add(g.hsum, (size_t)g.hcap * sizeof(unsigned long long));
    fl.add(g.hcnt, (size_t)g.hcap * sizeof(uint32_t));
    fl.launch(s);
  }
  const int bs = 256;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, 4096);
  hipLaunchKernelGGL(rag_ids_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, W, g);
  hipLaunchKernelGGL(rag_pad_kernel, dim3(256), dim3(bs), 0, s, g);
  BSMI_HIP(seg_sort_keys_u64(h->sort_tmp, h->sort_tmp_bytes, g.idu, g.ids, (int)g.node_cap, s));
  hipLaunchKernelGGL(rag_rank_kernel, dim3(256), dim3(bs), 0, s, g);
  hipLaunchKernelGGL(agg_edges_kernel<true>, dim3(grid), dim3(bs), 0, s, affs_dev, frags_dev, D, H, W, g);
  hipLaunchKernelGGL(rag_iota_kernel, dim3(1024), dim3(bs), 0, s, g);
  BSMI_HIP(seg_sort_pairs_u64_u32(h->sort_tmp, h->sort_tmp_bytes, g.hkeys, g.skeys, g.iota, g.sslot, (int)g.hcap, s));
  hipLaunchKernelGGL(rag_compact_kernel, dim3(std::min<uint32_t>(g.hcap / bs, 2048u)), dim3(bs), 0, s, g);
  hipLaunchKernelGGL(rag_merge_kernel, dim3(8), dim3(64), 0, s, g, threshold, discretize_queue, agg_fast_enabled() ? 1 : 0);
  return BSMI_OK;
}

int bsmi_rag_graph_u8(bsmi_seg* h, const uint8_t* affs_dev, const uint64_t* frags_dev, const int64_t shape[3], uint64_t* edges_dev,
                      uint64_t* sums_dev, uint32_t* pair_counts_dev, uint64_t edge_capacity, uint64_t* counts_dev, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !edges_dev || !sums_dev || !pair_counts_dev || !counts_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  hipStream_t s = (hipStream_t)stream;
  BSMI_HIP(hipSetDevice(h->device));
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  AggWs& g = h->agg;
  {
    Fills fl;
    fl.add(g.counters, 8 * sizeof(uint32_t));
    fl.add(counts_dev, 3 * sizeof(uint64_t));
    fl.add(g.idkeys, (size_t)g.icap * sizeof(uint64_t), 0xffffffffu);
    fl.add(g.hkeys, (size_t)g.hcap * sizeof(uint64_t), 0xffffffffu);
    fl.add(g.hsum, (size_t)g.hcap * sizeof(unsigned long long));
    fl.add(g.hcnt, (size_t)g.hcap * sizeof(uint32_t));
    fl.launch(s);
  }
  const int bs = 256;
  const int grid = (int)std::min<size_t>((n + bs - 1) / bs, 4096);
  hipLaunchKernelGGL(rag_ids_kernel, dim3(grid), dim3(bs), 0, s, frags_dev, n, (int)shape[2], g);
  hipLaunchKernelGGL(agg_edges_kernel<true>, dim3(grid), dim3(bs), 0, s, affs_dev, frags_dev, (int)shape[0], (int)shape[1], (int)shape[2], g);
  hipLaunchKernelGGL(rag_graph_hash_out_kernel, dim3(std::min<uint32_t>(g.hcap / bs, 2048u)), dim3(bs), 0, s, g, edges_dev, sums_dev, pair_counts_dev,
                     edge_capacity, counts_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_rag_merge_scores_u8(bsmi_seg* h, const uint8_t* affs_dev, const uint64_t* frags_dev, const int64_t shape[3],
                             float threshold, int discretize_queue, uint64_t* edges_dev, float* scores_dev,
                             uint64_t edge_capacity, uint64_t* merges_dev, float* merge_scores_dev, uint64_t* counts_dev,
                             void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev || !edges_dev || !scores_dev || !counts_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (discretize_queue < 1 || discretize_queue > kMaxQueueBins)
    BSMI_FAIL(BSMI_ERR_INVALID, "discretize_queue must be in [1, %d] (the exact-order queue is bsmi_agglomerate_mean_u8)", kMaxQueueBins);
  if (!(threshold > 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "threshold must be positive");
  hipStream_t s = (hipStream_t)stream;
  rc = rag_build_and_merge(h, affs_dev, frags_dev, shape, threshold, discretize_queue, counts_dev, s);
  if (rc) return rc;
  const int bs = 256;
  hipLaunchKernelGGL(rag_scores_kernel, dim3(1024), dim3(bs), 0, s, h->agg, edges_dev, scores_dev, edge_capacity, merges_dev,
                     merge_scores_dev, counts_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_rag_agglomerate_u8(bsmi_seg* h, const uint8_t* affs_dev, uint64_t* frags_dev, const int64_t shape[3], float threshold,
                            int discretize_queue, void* stream) {
  int rc = check_seg_shape(h, shape);
  if (rc) return rc;
  if (!affs_dev || !frags_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (discretize_queue < 1 || discretize_queue > kMaxQueueBins) BSMI_FAIL(BSMI_ERR_INVALID, "discretize_queue must be in [1, %d]", kMaxQueueBins);
  if (!(threshold > 0.f)) BSMI_FAIL(BSMI_ERR_INVALID, "threshold must be positive");
  hipStream_t s = (hipStream_t)stream;
  rc = rag_build_and_merge(h, affs_dev, frags_dev, shape, threshold, discretize_queue, nullptr, s);
  if (rc) return rc;
  const size_t n = (size_t)shape[0] * shape[1] * shape[2];
  hipLaunchKernelGGL(rag_relabel_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, frags_dev, n, h->agg);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_rag_edge_stats(bsmi_seg* h, uint64_t* sums_dev, uint64_t* counts_dev, uint64_t capacity, void* stream) {
  if (!h || !sums_dev || !counts_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(h->device));
  hipLaunchKernelGGL(rag_edge_stats_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, h->agg, sums_dev, counts_dev, capacity);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

// The segmentation workspace handle (create / destroy / status), the batch fill its users share, and the host-side connected
// components over a scored RAG.  The engine's file map and the handle's buffers: seg_internal.h.
#include <atomic>
#include <chrono>
#include <thread>

#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

// Several buffers set to a 32-bit pattern by ONE launch.  The runtime's fill (hipMemsetAsync) is a launch per buffer and a narrow one:
// the 33 MB sum table of the fragment filter took 0.84 ms beside the lanes' floods, the three tables together 1.7 ms of a block's
// 22 ms chain, and every launch is host time of the one thread that queues all lanes (kernel trace of the driver's job).
__device__ __forceinline__ void fill_list_body(const FillList& L) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int j = 0; j < L.n; ++j) {
    uint32_t* p = L.p[j];
    const size_t w = L.words[j];
    const uint32_t v = L.value[j];
    size_t head = (size_t)((0 - (uintptr_t)p) >> 2) & 3;  // words up to 16-byte alignment
    head = head < w ? head : w;
    if (t0 < head) p[t0] = v;
    uint4* q = (uint4*)(p + head);
    const size_t nv = (w - head) >> 2;
    for (size_t i = t0; i < nv; i += stride) q[i] = make_uint4(v, v, v, v);
    const size_t done = head + 4 * nv;
    if (t0 < w - done) p[done + t0] = v;
  }
}
__global__ __launch_bounds__(256) void fill_list_kernel(FillList L) { fill_list_body(L); }
__global__ __launch_bounds__(256) void fill_list_batch_kernel(const BatchBlock* __restrict__ tab) { fill_list_body(tab[blockIdx.y].fills); }
void Fills::launch(hipStream_t s) const {
  const unsigned grid = (unsigned)std::min<size_t>((most + 255) / 256 + 1, 2048);
  hipLaunchKernelGGL(fill_list_kernel, dim3(grid), dim3(256), 0, s, L);
}
void batch_fill_launch(const BatchBlock* tab, int N, size_t most, hipStream_t s) {
  const unsigned grid = (unsigned)std::min<size_t>((most + 255) / 256 + 1, 2048);
  hipLaunchKernelGGL(fill_list_batch_kernel, dim3(grid, N), dim3(256), 0, s, tab);
}

template <typename T>
static int dalloc(bsmi_seg* h, T** p, size_t count) {
  void* q = nullptr;
  BSMI_HIP(hipMalloc(&q, count * sizeof(T) + 16));
  h->allocs.push_back(q);
  *p = (T*)q;
  return BSMI_OK;
}
static uint32_t next_pow2(uint64_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

int check_seg_shape(bsmi_seg* h, const int64_t shape[3]) {
  if (!h || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (shape[d] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
  if ((size_t)shape[0] * shape[1] * shape[2] > h->max_vox || shape[0] > h->max_shape[0] ||
      shape[1] * shape[2] > h->max_shape[1] * h->max_shape[2])
    BSMI_FAIL(BSMI_ERR_INVALID, "shape (%lld,%lld,%lld) exceeds the handle's max_shape (%lld,%lld,%lld)",
              (long long)shape[0], (long long)shape[1], (long long)shape[2], (long long)h->max_shape[0],
              (long long)h->max_shape[1], (long long)h->max_shape[2]);
  return BSMI_OK;
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_seg_create(int device, const int64_t max_shape[3], bsmi_seg** out) {
  if (!max_shape || !out) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (max_shape[d] < 1 || max_shape[d] > 4096) BSMI_FAIL(BSMI_ERR_INVALID, "bad max_shape");
  BSMI_HIP(hipSetDevice(device));
  bsmi_seg* h = new bsmi_seg;
  h->device = device;
  for (int d = 0; d < 3; ++d) h->max_shape[d] = max_shape[d];
  const size_t nv = (size_t)max_shape[0] * max_shape[1] * max_shape[2];
  const size_t ns = (size_t)max_shape[1] * max_shape[2];
  h->max_vox = nv;
  int rc = 0;
#define A(ptr, cnt) if (!rc) rc = dalloc(h, &(ptr), (cnt))
  A(h->ws.mask, nv); A(h->ws.g, nv); A(h->ws.d2, nv); A(h->ws.mf, nv); A(h->ws.par, nv); A(h->ws.lab, nv);
  A(h->ws.nseeds, (size_t)max_shape[0]); A(h->ws.offs, (size_t)max_shape[0]);
  h->ws.seedlab = nullptr;
  h->flood_spill_stride = ns;
  A(h->flood_spill, nv);
  if (ns >= ((size_t)1 << 20)) A(h->flood_spill_idx, nv);  // (the wide flood's keys spill into flood_spill)
  AggWs& g = h->agg;
  static std::atomic<int> next_xcd{0};
  g.xcd_hint = next_xcd.fetch_add(1) & 7;
  g.id_cap = (uint32_t)std::min<size_t>(nv + 2, (size_t)1 << 27);
  g.node_cap = (uint32_t)std::min<size_t>(nv / 8 + 1024, (size_t)1 << 24);
  g.hcap = next_pow2(std::max<size_t>(nv / 2, 1024));
  g.edge_cap = g.hcap / 2;
  A(g.rank_of_id, (size_t)g.id_cap); A(g.ids, (size_t)g.node_cap); A(g.counters, 8);
  A(g.hkeys, (size_t)g.hcap); A(g.hvals, (size_t)g.hcap); A(g.hsum, (size_t)g.hcap); A(g.hcnt, (size_t)g.hcap);
  A(g.eu, (size_t)g.edge_cap); A(g.ev, (size_t)g.edge_cap); A(g.ekey0, (size_t)g.edge_cap);
  A(g.esum, (size_t)g.edge_cap); A(g.ecnt, (size_t)g.edge_cap); A(g.enextu, (size_t)g.edge_cap);
  A(g.enextv, (size_t)g.edge_cap); A(g.eflags, (size_t)g.edge_cap);
  A(g.head, (size_t)g.node_cap); A(g.parent, (size_t)g.node_cap);
  A(g.roots, (size_t)g.node_cap * kMaxThresholds); A(g.heap_spill, (size_t)g.edge_cap); A(g.maxid, 1);
  A(g.sticky, 1);
  A(g.escore, (size_t)g.edge_cap); A(g.etime, (size_t)g.edge_cap); A(g.ntime, (size_t)g.node_cap);
  A(h->thr_dev, kMaxThresholds); A(h->status_dev, 4);
  FragWs& f = h->frag;
  f.id_cap = (uint32_t)std::min<size_t>(nv + 2, (size_t)1 << 27);
  A(f.lsum, (size_t)f.id_cap); A(f.lcnt, (size_t)f.id_cap); A(f.rank, nv); A(f.blk, nv / 1024 + 2); A(f.flags, 4);
  f.par = h->ws.par;
  A(h->crop_tmp, nv);
  g.icap = next_pow2((size_t)g.node_cap * 2);
  A(g.idkeys, (size_t)g.icap); A(g.idvals, (size_t)g.icap); A(g.idu, (size_t)g.node_cap);
  A(g.skeys, (size_t)g.hcap); A(g.sslot, (size_t)g.hcap); A(g.iota, (size_t)g.hcap); A(g.qnext, (size_t)g.edge_cap);
  A(g.tnext, (size_t)g.node_cap * 2); A(g.tscore, (size_t)g.node_cap * 2); A(g.cur, (size_t)g.node_cap);
  A(g.ha, (size_t)g.node_cap); A(g.hb, (size_t)g.node_cap); A(h->rag_counts, 4);
  A(g.tcount, (size_t)g.icap); A(g.tzmin, (size_t)g.icap); A(g.tzmax, (size_t)g.icap);
  if (!rc) {
    size_t b = 0;
    if (seg_sort_tmp_bytes((int)g.node_cap, (int)g.hcap, &b) != hipSuccess) {
      bsmi::set_error("hipcub temp-storage query failed");
      rc = BSMI_ERR_HIP;
    } else {
      h->sort_tmp_bytes = b + 256;
      uint8_t* t = nullptr;
      rc = dalloc(h, &t, h->sort_tmp_bytes);
      h->sort_tmp = t;
    }
  }
#undef A
  if (rc) {
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
    return rc;
  }
  BSMI_HIP(hipMemset(g.counters, 0, 8 * sizeof(uint32_t)));
  BSMI_HIP(hipMemset(g.sticky, 0, sizeof(uint32_t)));
  BSMI_HIP(hipMemset(h->frag.flags, 0, 4 * sizeof(uint32_t)));
  BSMI_HIP(hipDeviceSynchronize());  // the fills ran on the null stream; the lanes' streams are non-blocking and would not wait for them
  *out = h;
  return BSMI_OK;
}

int bsmi_seg_destroy(bsmi_seg* h) {
  if (!h) return BSMI_OK;
  (void)hipSetDevice(h->device);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return BSMI_OK;
}

// Host-side union-find over the scored RAG (reference post/watershed.py:182,
// funlib.segment.graphs.impl.connected_components [EXT]); same contract as oracle seg_connected_components:
// score <= threshold joins, a component is named by its smallest node id, nodes ascending.
int bsmi_connected_components_multi(const uint64_t* nodes, uint64_t n, const uint64_t* edges, const float* scores, uint64_t m,
                                    const float* thresholds, int n_thresholds, uint64_t* components) {
  if ((n && (!nodes || !components)) || (m && (!edges || !scores)) || !thresholds || n_thresholds < 1)
    BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n >= 0xffffffffull) BSMI_FAIL(BSMI_ERR_INVALID, "%llu nodes: the union-find indices are 32-bit", (unsigned long long)n);
  for (uint64_t i = 1; i < n; ++i)
    if (nodes[i] <= nodes[i - 1]) BSMI_FAIL(BSMI_ERR_INVALID, "nodes must be strictly ascending");
  // node ids -> indices, once for all thresholds, on a few host threads (two binary searches per edge)
  constexpr uint32_t kNone = 0xffffffffu;
  const double t_begin = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  std::vector<uint32_t> iu(m), iv(m);
  {
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const unsigned T = m < 20000 ? 1u : hw;  // 143 000 edges on one thread: 5 ms of the job's last 9
    // two-level search: every 64th id in a table that stays in cache, then the 64 ids of one run (8 cache lines)
    constexpr uint64_t kRun = 64;
    std::vector<uint64_t> coarse((n + kRun - 1) / kRun);
    for (size_t c = 0; c < coarse.size(); ++c) coarse[c] = nodes[c * kRun];
    auto index_of = [&](uint64_t id) -> uint32_t {
      if (!n || id < nodes[0]) return kNone;
      const size_t c = (size_t)(std::upper_bound(coarse.begin(), coarse.end(), id) - coarse.begin()) - 1;
      const uint64_t* lo = nodes + c * kRun;
      const uint64_t* hi = nodes + std::min<uint64_t>(n, (c + 1) * kRun);
      const uint64_t* p = std::lower_bound(lo, hi, id);
      return (p != hi && *p == id) ? (uint32_t)(p - nodes) : kNone;
    };
    auto work = [&](uint64_t e0, uint64_t e1) {
      for (uint64_t e = e0; e < e1; ++e) {
        const uint32_t a = index_of(edges[2 * e]), b = index_of(edges[2 * e + 1]);
        const bool ok = a != kNone && b != kNone;
        iu[e] = ok ? a : kNone;
        iv[e] = ok ? b : kNone;
      }
    };
    if (T == 1) {
      work(0, m);
    } else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < T; ++t) th.emplace_back(work, m * t / T, m * (t + 1) / T);
      for (auto& x : th) x.join();
    }
  }
  const bool dbg = getenv("BSMI_CC_DEBUG") != nullptr;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_map = now();
  if (dbg) fprintf(stderr, "[cc] look-up of %llu edges: %.3f s\n", (unsigned long long)m, t_map - t_begin);
  std::vector<uint32_t> parent(n);
  for (uint64_t i = 0; i < n; ++i) parent[i] = (uint32_t)i;
  auto find = [&](uint32_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  // thresholds in ascending order: the edges of a lower threshold are among those of a higher one, and with the smaller
  // index as the root a component's name does not depend on the order of the unions
  std::vector<int> order(n_thresholds);
  for (int k = 0; k < n_thresholds; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return thresholds[a] < thresholds[b]; });
  float prev = -INFINITY;
  bool first = true;
  for (int k : order) {
    const float t = thresholds[k];
    for (uint64_t e = 0; e < m; ++e) {
      const float sc = scores[e];
      if (!(sc <= t) || (!first && sc <= prev) || iu[e] == kNone) continue;
      const uint32_t a = find(iu[e]), b = find(iv[e]);
      if (a == b) continue;
      if (a < b) parent[b] = a; else parent[a] = b;
    }
    const double t_un = now();
    uint64_t* out = components + (size_t)k * n;
    for (uint64_t i = 0; i < n; ++i) out[i] = nodes[find((uint32_t)i)];
    if (dbg) fprintf(stderr, "[cc] threshold %g: unions until %.3f, snapshot %.3f s\n", t, t_un - t_map, now() - t_un);
    prev = t;
    first = false;
  }
  return BSMI_OK;
}

int bsmi_connected_components(const uint64_t* nodes, uint64_t n, const uint64_t* edges, const float* scores, uint64_t m,
                              float threshold, uint64_t* components) {
  return bsmi_connected_components_multi(nodes, n, edges, scores, m, &threshold, 1, components);
}

int bsmi_seg_set_host_flood(bsmi_seg* h, int on) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  h->host_flood3 = on != 0;
  return BSMI_OK;
}

int bsmi_seg_status(bsmi_seg* h, void* stream) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  BSMI_HIP(hipSetDevice(h->device));
  uint32_t c[8], sticky = 0;
  BSMI_HIP(hipMemcpyAsync(c, h->agg.counters, sizeof c, hipMemcpyDeviceToHost, (hipStream_t)stream));
  BSMI_HIP(hipMemcpyAsync(&sticky, h->agg.sticky, sizeof sticky, hipMemcpyDeviceToHost, (hipStream_t)stream));
  BSMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  uint32_t ff[4];
  BSMI_HIP(hipMemcpy(ff, h->frag.flags, sizeof ff, hipMemcpyDeviceToHost));
  if (ff[0]) BSMI_FAIL(BSMI_ERR_OVERFLOW, "fragment id exceeds the post-processing table (ids must stay below %u)", h->frag.id_cap);
  // counters[3]: the last call; sticky: every call on this handle since the previous status check (cleared here)
  const uint32_t flags = c[3] | sticky;
  if (sticky) BSMI_HIP(hipMemsetAsync(h->agg.sticky, 0, sizeof(uint32_t), (hipStream_t)stream));
  if (flags)
    BSMI_FAIL(BSMI_ERR_OVERFLOW, "agglomeration workspace overflow (flags 0x%x: 1 id range, 2 nodes, 4 hash, 8 edges, 16 hash churn, 32 edge buffer too small)", flags);
  return BSMI_OK;
}

}  // extern "C"

// Segmentation half of the hot path on gfx950: seeded-watershed fragments
// (reference post/ws.py:8-112) and mean-affinity hierarchical agglomeration (reference call
// site post/watershed.py:333-338; algorithm specified in oracle/seg_ref.c).
//
// Everything is integer work held bit-exact to the oracle:
//   fragments (fragments_in_xy): one workgroup per z-slice computes the foreground mask
//     (a_y + a_x >= 256), the exact squared EDT, the separable reflect-border max filter,
//     the maxima, their 4-connected components numbered in raster order; a tiny scan gives
//     the running id offset of ws.py:74-92; then one wave per slice replays skimage's
//     priority flood exactly (binary heap keyed (value, age), label-at-push) with the heap in
//     LDS -- the flood order is inherently sequential per slice, the parallelism is across
//     the slices (128 per block, 65,536 per 1024^3 volume).
//   agglomeration: region-adjacency graph by parallel scan + device hash table (sum, count
//     per edge), then one wave per volume replays the specified sequential merge loop
//     (min-queue over the total order (score, initial edge key)), then a parallel relabel.
//
// This header is what the translation units of the engine share: the workspace handle and its parts, a few device helpers,
// and the host launchers one file exports to another.  A kernel lives in the file that launches it:
//   seg.hip         the handle (create / destroy / status), the fill of several buffers by one launch, the host-side connected components
//   seg_ws.hip      fragments, xy mode: seeds, offsets, the compact / plain / wide floods; the public fragments entry
//   seg_ws3.hip     fragments, 3-D mode: EDT, max filter, markers, the single-wave flood and the hand-off to flood_host.cpp
//   seg_graph.hip   agg_* (mean / histogram agglomeration) and rag_* (blockwise edge scoring) and their entry points
//   seg_labels.hip  LUT relabel, fragment clean-up, the connected-components family, label statistics, the label table
//   seg_sort.hip    the radix sorts (the only file that includes hipcub)
//   seg_batch.hip   the batch object: a table of workspaces in device memory and the two entry points that serve every block
//                   of a stage with one launch per kernel (the kernels' batched forms sit beside their single-block forms)
#pragma once
#include <vector>

#include "common.h"
#include "u64_table.h"  // mix64: the hash of every open-addressing table here

namespace bsmi {

constexpr uint64_t HEMPTY = 0xffffffffffffffffull;
constexpr uint64_t HTOMB = 0xfffffffffffffffeull;
constexpr uint32_t NOEDGE = 0xffffffffu;
constexpr int kMaxThresholds = 16;

__device__ __forceinline__ int reflect_dup(int i, int n) {
  const int p = 2 * n;
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - 1 - i;
}
// the same for -n <= i < 2 n (a filter window no wider than the axis), without the division
__device__ __forceinline__ int reflect_near(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// scratch per slice (global memory, L2 resident): mask u8, g/d2/mf int32, parent int32, lab int32.  The 3-D mode uses the same
// arrays as whole-volume ones (g and mf: ping-pong buffers of the EDT and the max filter).
struct WsScratch {
  uint8_t* mask;
  int32_t* g;
  int32_t* d2;
  int32_t* mf;
  int32_t* par;     // ALSO FragWs::par: every connected-components pass of the handle writes it (see bsmi_seg)
  int32_t* lab;     // local seed labels (1..n), later flood labels
  int32_t* nseeds;  // [D]
  uint64_t* offs;   // [D] exclusive scan of nseeds
  int32_t* seedlab; // optional (return_seeds): the seed labels before masking (ws.py:20-23), slice-local numbering
};

// Workspace of the region graph and its merge loops.  One set of tables, three users that each start by zeroing `counters`
// and clearing the tables they fill: the mean / histogram agglomeration (agg_*), the RAG path (rag_*) and the label table of
// `bs refine` (ltab_*).  Passed to the kernels BY VALUE: the layout below is their argument layout.
struct AggWs {
  // node table
  uint32_t* rank_of_id;  // [id_cap]: direct-address table id -> rank (after scan), 0xffffffff = absent
  uint32_t id_cap;
  uint64_t* ids;         // [node_cap] rank -> id (agg, rag); label table: the ids ascending (output of its sort)
  uint32_t node_cap;
  uint32_t* counters;    // [0]=nn, [1]=ne, [2]=heap_n, [3]=overflow flags of the call in flight (zeroed by every call)
                         // [4]=merges of the RAG loop, [5],[6]=xcd_claim's claim / arrivals, [7]=edge ranks valid (mean path)
  uint32_t* sticky;      // [1] overflow flags of every call since the last bsmi_seg_status (the last kernel of a call ORs [3] in)
  // hash table over edges
  uint64_t* hkeys;       // [hcap]
  uint32_t* hvals;       // [hcap] -> edge index
  unsigned long long* hsum;  // [hcap] (during build)
  uint32_t* hcnt;        // [hcap]
  uint32_t hcap;         // power of two
  // edge arrays [edge_cap]
  uint32_t* eu; uint32_t* ev; uint64_t* ekey0; unsigned long long* esum; uint32_t* ecnt;
  uint32_t* enextu; uint32_t* enextv; uint8_t* eflags;  // bit0 deleted, bit1 stale
  uint32_t edge_cap;
  uint32_t* head;        // [node_cap]
  uint32_t* parent;      // [node_cap]
  uint32_t* roots;       // [nthr_cap][node_cap]
  uint64_t* heap_spill;  // [edge_cap]
  uint64_t* maxid;       // [1]
  // RAG scoring path (arbitrary 64-bit ids): id hash, sorted edge numbering, bin queue, merge tree
  uint64_t* idkeys;      // [icap] open-addressing set of fragment ids (rag_ids_kernel); label table: its id set (ltab_scan_kernel)
  uint32_t* idvals;      // [icap] -> rank
  uint32_t icap;         // power of two
  uint64_t* idu;         // [node_cap] distinct ids before sorting (rag and label table alike)
  uint64_t* skeys;       // [hcap] edge keys sorted
  uint32_t* sslot;       // [hcap] hash slot of the sorted key (read again by bsmi_rag_edge_stats after the call)
  uint32_t* iota;        // [hcap]
  uint32_t* qnext;       // [edge_cap] FIFO links of the bin queue; mean path: the edges' ranks by initial key (agg_edge_rank_kernel)
  uint32_t* tnext;       // [2 * node_cap] merge tree parent
  float* tscore;         // [2 * node_cap]
  uint32_t* cur;         // [node_cap] tree node of a cluster root
  uint32_t* ha; uint32_t* hb;  // [node_cap] merge history (ranks); label table: idkeys slot of an id before (ha) / after (hb) its sort
  float* escore;         // [edge_cap] stored score: the score at the edge's last (re)scoring = its place in the queue
  uint32_t* etime;       // [edge_cap] RAG path: merge clock at the edge's last scoring
  uint32_t* ntime;       // [node_cap] RAG path: merge clock when the node last survived a merge (edges scored before are stale)
  int xcd_hint;          // XCD the sequential merge loop of this workspace should run on (see xcd_claim)
  // label table (bs refine): per id-hash slot.  Written and read by the ltab_* kernels alone (bsmi_label_table_u64); they sit
  // here, not in a struct of their own, because those kernels take the whole AggWs (idkeys, idu, ids, ha, hb, counters).
  unsigned long long* tcount;  // [icap]
  int* tzmin; int* tzmax;      // [icap]
};

// Last kernel of a call: an overflow of this call outlives the next call's reset of counters[3] (a pipeline that checks
// bsmi_seg_status once per lane after many blocks must still see it).
__device__ __forceinline__ void keep_overflow(const AggWs& w) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t f = w.counters[3];
    if (f) atomicOr(w.sticky, f);
  }
}

// fragment clean-up and the connected-components passes
struct FragWs {
  unsigned long long* lsum;  // [id_cap] sum of a_z + a_y + a_x over the voxels of a fragment
  uint32_t* lcnt;            // [id_cap] voxel count
  uint32_t id_cap;
  int32_t* par;              // [max_vox] union-find parent (crop volume) -- the SAME array as WsScratch::par
  int32_t* rank;             // [max_vox] raster-order rank of a root
  uint32_t* blk;             // [max_vox / 1024 + 2] per-block root counts / offsets
  uint32_t* flags;           // [0] overflow (id >= id_cap)
};

// Union-find over voxel indices, the smaller index wins (int32_t parents, atomicMin).  csrc/morph.hip's uf_find / uf_unite are
// a different algorithm (uint32_t, compare-and-swap) and stay separate.
__device__ __forceinline__ int cc_find(int32_t* par, int a) {
  int p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != a) {
    a = p;
    p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return a;
}
__device__ __forceinline__ void cc_unite(int32_t* par, int a, int b) {
  for (;;) {
    a = cc_find(par, a);
    b = cc_find(par, b);
    if (a == b) break;
    const int hi = a < b ? b : a, lo = a < b ? a : b;  // the larger root is hung under the smaller one
    const int old = atomicMin(&par[hi], lo);
    if (old == hi) break;  // else hi was no root any more: go on from what it pointed at
    a = old;
    b = lo;
  }
}

// Several buffers set to a 32-bit pattern by ONE launch (fill_list_kernel, seg.hip).
constexpr int kMaxFills = 6;
struct FillList {
  uint32_t* p[kMaxFills];
  size_t words[kMaxFills];
  uint32_t value[kMaxFills];
  int n;
};
struct Fills {
  FillList L{};
  size_t most = 0;
  void add(void* p, size_t bytes, uint32_t value = 0) {  // 4-byte aligned, whole words (every table here is)
    L.p[L.n] = (uint32_t*)p; L.words[L.n] = bytes / 4; L.value[L.n] = value; ++L.n;
    most = std::max(most, bytes / 16);
  }
  void launch(hipStream_t s) const;
};

// ---- batched calls (seg_batch.hip): N blocks of one read shape per launch -------------------------------------------------
// A kernel's body is a __device__ function with the single-block kernel's arguments; the batched __global__ takes them from
// table[blockIdx.y] and calls the same body, so a block's arithmetic is the single-block form's by construction.
constexpr int kMaxBatch = 32;
// per-call arguments of one block (include/bsmi.h: bsmi_batch_frag_args / bsmi_batch_graph_args, the same layout)
struct BatchFragArgs {
  const uint8_t* affs; uint64_t* frags; uint64_t* max_id; uint64_t* labels; uint64_t* num; uint64_t id_offset;
  uint64_t* size; uint64_t* sums;
};
struct BatchGraphArgs {
  const uint8_t* affs; const uint64_t* frags; uint64_t* edges; uint64_t* sums; uint32_t* pair_counts; uint64_t* counts;
  uint64_t edge_capacity;
};
// One row of the table: a handle's workspaces (written once, when the batch object is created) and the arguments and fill
// lists of the call in flight (written by the call's first launch, in stream order: a call queued behind another cannot
// overwrite what the earlier one still reads).
struct BatchBlock {
  WsScratch ws;  // seedlab = nullptr
  uint64_t* flood_spill;
  size_t flood_spill_stride;
  int* status;
  FragWs frag;
  uint64_t* crop_tmp;
  AggWs agg;
  BatchFragArgs f;
  BatchGraphArgs g;
  FillList fills;
};

}  // namespace bsmi

// The handle.  Every buffer is allocated once, by bsmi_seg_create, for max_shape; the entry points share them WITHOUT any
// locking or ordering of their own, so what follows is the whole rule.
//
// Who uses what (entry points by the buffers they write):
//   F   bsmi_ws_fragments(_seeds)_u8, both modes      ws.* (all of it), flood_spill, flood_spill_idx, seedlab, status_dev;
//                                                     the 3-D mode also frag.par (= ws.par), frag.rank, frag.blk, crop_tmp
//   C   bsmi_frag_postprocess_u8, bsmi_cc_affs_u8     frag.* (so ws.par), crop_tmp
//   G   bsmi_agglomerate_mean_u8 / _hist_u8,          agg.* (each call zeroes agg.counters and clears the tables it fills),
//       bsmi_rag_graph_u8, bsmi_rag_merge_scores_u8,  sort_tmp (the RAG calls and the label table)
//       bsmi_rag_agglomerate_u8, bsmi_label_table_u64
//       bsmi_rag_edge_stats                           reads agg.sslot / hsum / hcnt / counters as the last RAG call left them
//       bsmi_seg_status                               reads agg.counters, agg.sticky (and clears it), frag.flags
//   bsmi_label_stats, bsmi_lut_relabel(_multi) touch no buffer of the handle.
//
//   a batched call (bsmi_seg_batch_fragments_u8: F and C; bsmi_seg_batch_rag_graph_u8: G) uses those buffers of EVERY handle
//   the batch object was created from, for the blocks it is given and also for none (its launches cover all rows it is told).
//
// Which calls must not be in flight together on one handle: any two of F and C (they share ws.par and crop_tmp, also a call
// with itself), and any two of G (also a call with itself).  A call of G shares no device buffer with F or C.  "In flight
// together" means on different streams without an event between them, or from two host threads: the host side of a call is
// not thread-safe either (seedlab is allocated on first use, host_flood3 is a plain flag).  Every caller in this project
// gives a handle to one host thread and one stream (post/engine.py: "one per host thread per GPU"), where all of this holds
// by stream order; bsmi_rag_edge_stats and bsmi_seg_status then see the call queued before them.
struct bsmi_seg {
  int device = 0;
  int64_t max_shape[3] = {0, 0, 0};
  size_t max_vox = 0;
  std::vector<void*> allocs;
  bsmi::WsScratch ws{};
  // [max_vox] heap entries past the LDS part: per slice (flood_spill_stride apart) of ws_flood_kernel, the keys of
  // ws_flood_wide_kernel, the whole volume's of ws3_flood_kernel
  uint64_t* flood_spill = nullptr;
  size_t flood_spill_stride = 0;
  uint32_t* flood_spill_idx = nullptr;  // [max_vox] voxel indices of ws_flood_wide_kernel's spilled entries (slices of 2^20 voxels and more only)
  bsmi::AggWs agg{};
  bsmi::FragWs frag{};  // frag.par == ws.par (set by bsmi_seg_create)
  // [max_vox] three uses: the cropped fragments before relabelling (bsmi_frag_postprocess_u8: crop_u64_kernel writes, the cc26
  // kernels read), the per-voxel `touched` flags of bsmi_cc_affs_u8 (ccaff_* write, cc26_write_kernel reads them as the value
  // array), and the maxima flags of the 3-D fragments mode (ws3_maxima_kernel writes, cc6_union / ws3_markers read)
  uint64_t* crop_tmp = nullptr;
  void* sort_tmp = nullptr;      // radix-sort scratch (seg_sort.hip), sized for the larger of the two sorts
  size_t sort_tmp_bytes = 0;
  int32_t* seedlab = nullptr;      // [max_vox] unmasked seed labels (bsmi_ws_fragments_seeds_u8), allocated on first use
  uint64_t* rag_counts = nullptr;  // [4] allocated, not used by any entry point (the RAG calls write the caller's counts_dev)
  float* thr_dev = nullptr;        // [kMaxThresholds] allocated, not used (thresholds travel by value: AggThresholds)
  // [4] ints: [0] is `any_bg` of the 3-D fragments mode (zeroed, ws3_mask_kernel ORs, ws3_edt_nobg_kernel reads); the xy floods
  // take the pointer as their `status` argument and do not touch it
  int* status_dev = nullptr;
  bool host_flood3 = false;  // bsmi_seg_set_host_flood: the 3-D watershed's flood runs on the host (flood_host.cpp)
};

namespace bsmi {

// seg.hip
int check_seg_shape(bsmi_seg* h, const int64_t shape[3]);

// seg_ws3.hip: the 3-D fragments mode (fragments_in_xy = 0) behind bsmi_ws_fragments_seeds_u8, arguments already validated
int fragments_3d(bsmi_seg* h, const uint8_t* affs_dev, int D, int H, int W, int min_seed_distance, uint64_t* frags_dev,
                 uint64_t* max_id_dev, uint64_t* seeds_dev, hipStream_t s);

// the batched launchers (arguments validated by seg_batch.hip; `tab` = device table, rows 0..N-1 in use)
// seg.hip: every row's `fills` in one launch; `most` = 16-byte units of the largest buffer among them
void batch_fill_launch(const BatchBlock* tab, int N, size_t most, hipStream_t s);
// seg_ws.hip: is (H, W) on the LDS / compact path (the only one the batch serves)?  -> the seed kernel's LDS bytes, 0 = no
size_t batch_ws_lds_bytes(int H, int W);
int batch_ws_launch(const BatchBlock* tab, int N, int D, int H, int W, int msd, hipStream_t s);
// seg_labels.hip: clean-up, crop, 26-connected relabel, label statistics
void batch_post_launch(const BatchBlock* tab, int N, const int64_t shape[3], double filter_value, int64_t min_size, const int64_t crop_offset[3],
                       const int64_t crop_shape[3], uint64_t stats_num, hipStream_t s);
// seg_graph.hip: ids, edges, the graph out of the hash table
void batch_graph_launch(const BatchBlock* tab, int N, const int64_t shape[3], uint32_t max_hcap, hipStream_t s);

// seg_labels.hip: raster-order ranks of the union-find roots in f.par (cc26_count / cc26_scan / cc26_rank), their number
// to *num_out
void cc_rank_roots(size_t n, const FragWs& f, uint64_t* num_out, hipStream_t s);

// seg_sort.hip: radix sorts over all 64 key bits; `tmp` holds at least what seg_sort_tmp_bytes reported
hipError_t seg_sort_tmp_bytes(int n_keys, int n_pairs, size_t* bytes);  // the larger need of a key sort and a pair sort
hipError_t seg_sort_keys_u64(void* tmp, size_t tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, int n, hipStream_t s);
hipError_t seg_sort_pairs_u64_u32(void* tmp, size_t tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in,
                                  uint32_t* vals_out, int n, hipStream_t s);

}  // namespace bsmi

// The batch object: every block of a segmentation stage per launch.  A pipeline that runs a block's chain of ~19 short launches
// on a stream of its own per block gets as many chains side by side as the runtime grants hardware queues (HIP's default: 4);
// here a stage's concurrency is the grid's: launch (x, block) of a kernel serves workgroup x of block `block`, whose workspace
// and arguments it finds in row `block` of a table in device memory.  The kernels are the single-block ones (their bodies are
// shared: seg_internal.h), the workspaces are existing handles, one per row.
//
// Served: the default blockwise path -- xy fragments on the LDS / compact path, fragment filter / debris removal, crop,
// 26-connected relabel, label statistics; the region graph for host-side scoring.  Everything else (3-D mode, return_seeds,
// slices off the LDS path, the device merge loops) is refused with BSMI_ERR_INVALID: the caller runs it handle by handle.
//
// No call here synchronises with the host or copies from host memory: the per-call arguments (64 bytes per block) travel as
// kernel arguments of the call's first launch, which writes them into the table -- in stream order, so a call queued behind
// another one cannot overwrite rows the earlier call's launches still read.
#include "seg_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

struct bsmi_seg_batch {
  int device = 0;
  int n = 0;
  std::vector<bsmi_seg*> handles;
  bsmi::BatchBlock* tab = nullptr;  // [n] device
  uint32_t max_frag_id_cap = 0, max_icap = 0, max_hcap = 0;
};

namespace bsmi {

static_assert(sizeof(BatchFragArgs) == sizeof(bsmi_batch_frag_args) && sizeof(BatchGraphArgs) == sizeof(bsmi_batch_graph_args),
              "include/bsmi.h and seg_internal.h disagree on the per-block arguments");

struct BatchFragCall { BatchFragArgs a[kMaxBatch]; };
struct BatchGraphCall { BatchGraphArgs a[kMaxBatch]; };

// first launch of a fragments call: row blockIdx.x takes its arguments and the list of what bsmi_frag_postprocess_u8 and
// bsmi_label_stats clear before they start
__global__ __launch_bounds__(64) void batch_set_frag_kernel(BatchBlock* tab, BatchFragCall c, uint64_t stats_num, int with_filter) {
  if (threadIdx.x != 0) return;
  BatchBlock& b = tab[blockIdx.x];
  const BatchFragArgs a = c.a[blockIdx.x];
  b.f = a;
  FillList L{};
  L.p[0] = b.frag.flags; L.words[0] = 4;
  L.p[1] = (uint32_t*)a.size; L.words[1] = 2 * (size_t)stats_num;
  L.p[2] = (uint32_t*)a.sums; L.words[2] = 6 * (size_t)stats_num;
  L.n = 3;
  if (with_filter) {
    L.p[3] = (uint32_t*)b.frag.lsum; L.words[3] = 2 * (size_t)b.frag.id_cap;
    L.p[4] = b.frag.lcnt; L.words[4] = (size_t)b.frag.id_cap;
    L.n = 5;
  }
  b.fills = L;
}

// ... of a graph call: what bsmi_rag_graph_u8 clears
__global__ __launch_bounds__(64) void batch_set_graph_kernel(BatchBlock* tab, BatchGraphCall c) {
  if (threadIdx.x != 0) return;
  BatchBlock& b = tab[blockIdx.x];
  const BatchGraphArgs a = c.a[blockIdx.x];
  b.g = a;
  FillList L{};
  L.p[0] = b.agg.counters; L.words[0] = 8;
  L.p[1] = (uint32_t*)a.counts; L.words[1] = 6;
  L.p[2] = (uint32_t*)b.agg.idkeys; L.words[2] = 2 * (size_t)b.agg.icap; L.value[2] = 0xffffffffu;
  L.p[3] = (uint32_t*)b.agg.hkeys; L.words[3] = 2 * (size_t)b.agg.hcap; L.value[3] = 0xffffffffu;
  L.p[4] = (uint32_t*)b.agg.hsum; L.words[4] = 2 * (size_t)b.agg.hcap;
  L.p[5] = b.agg.hcnt; L.words[5] = (size_t)b.agg.hcap;
  L.n = 6;
  b.fills = L;
}

static int batch_check(bsmi_seg_batch* b, int n_blocks, const void* args, const int64_t shape[3]) {
  if (!b || !args || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n_blocks < 1 || n_blocks > b->n) BSMI_FAIL(BSMI_ERR_INVALID, "%d blocks for a batch of %d workspaces", n_blocks, b->n);
  for (int i = 0; i < n_blocks; ++i) {
    const int rc = check_seg_shape(b->handles[i], shape);
    if (rc) return rc;
  }
  if (shape[1] > 4096 || shape[2] > 4096 || !batch_ws_lds_bytes((int)shape[1], (int)shape[2]))
    BSMI_FAIL(BSMI_ERR_INVALID, "slices of %lld x %lld are off the LDS / compact path: not served in batches", (long long)shape[1],
              (long long)shape[2]);
  return BSMI_OK;
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_seg_batch_create(bsmi_seg* const* handles, int n, bsmi_seg_batch** out) {
  if (!handles || !out) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (n < 1 || n > kMaxBatch) BSMI_FAIL(BSMI_ERR_INVALID, "a batch takes 1 to %d workspaces (got %d)", kMaxBatch, n);
  for (int i = 0; i < n; ++i) {
    if (!handles[i]) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
    if (handles[i]->device != handles[0]->device) BSMI_FAIL(BSMI_ERR_INVALID, "the workspaces of a batch must be on one device");
    for (int j = 0; j < i; ++j)
      if (handles[j] == handles[i]) BSMI_FAIL(BSMI_ERR_INVALID, "a workspace appears twice in the batch");
  }
  BSMI_HIP(hipSetDevice(handles[0]->device));
  bsmi_seg_batch* b = new bsmi_seg_batch;
  b->device = handles[0]->device;
  b->n = n;
  b->handles.assign(handles, handles + n);
  std::vector<BatchBlock> rows(n);
  for (int i = 0; i < n; ++i) {
    const bsmi_seg* h = handles[i];
    BatchBlock& r = rows[i];
    r = BatchBlock{};
    r.ws = h->ws;
    r.ws.seedlab = nullptr;
    r.flood_spill = h->flood_spill;
    r.flood_spill_stride = h->flood_spill_stride;
    r.status = h->status_dev;
    r.frag = h->frag;
    r.crop_tmp = h->crop_tmp;
    r.agg = h->agg;
    b->max_frag_id_cap = std::max(b->max_frag_id_cap, h->frag.id_cap);
    b->max_icap = std::max(b->max_icap, h->agg.icap);
    b->max_hcap = std::max(b->max_hcap, h->agg.hcap);
  }
  void* q = nullptr;
  hipError_t err = hipMalloc(&q, sizeof(BatchBlock) * n);
  if (err == hipSuccess) err = hipMemcpy(q, rows.data(), sizeof(BatchBlock) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipDeviceSynchronize();  // (as bsmi_seg_create: the callers' streams are non-blocking)
  if (err != hipSuccess) {
    if (q) (void)hipFree(q);
    delete b;
    BSMI_HIP(err);
  }
  b->tab = (BatchBlock*)q;
  *out = b;
  return BSMI_OK;
}

int bsmi_seg_batch_destroy(bsmi_seg_batch* b) {
  if (!b) return BSMI_OK;
  (void)hipSetDevice(b->device);
  if (b->tab) (void)hipFree(b->tab);
  delete b;
  return BSMI_OK;
}

int bsmi_seg_batch_fragments_u8(bsmi_seg_batch* b, int n_blocks, const bsmi_batch_frag_args* args, const int64_t shape[3],
                                int fragments_in_xy, int min_seed_distance, double filter_value, int64_t min_size,
                                const int64_t crop_offset[3], const int64_t crop_shape[3], uint64_t stats_num, void* stream) {
  int rc = batch_check(b, n_blocks, args, shape);
  if (rc) return rc;
  if (!fragments_in_xy) BSMI_FAIL(BSMI_ERR_INVALID, "the 3-D fragments mode is not served in batches");
  if (min_seed_distance < 1 || min_seed_distance > 64) BSMI_FAIL(BSMI_ERR_INVALID, "min_seed_distance out of range");
  if (!crop_offset || !crop_shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (crop_offset[d] < 0 || crop_shape[d] < 1 || crop_offset[d] + crop_shape[d] > shape[d])
      BSMI_FAIL(BSMI_ERR_INVALID, "crop outside the fragment volume");
  BatchFragCall call{};
  for (int i = 0; i < n_blocks; ++i) {
    const bsmi_batch_frag_args& a = args[i];
    if (!a.affs_dev || !a.frags_dev || !a.max_id_dev || !a.labels_dev || !a.num_labels_dev || !a.size_dev || !a.sums_dev)
      BSMI_FAIL(BSMI_ERR_INVALID, "null argument (block %d)", i);
    call.a[i] = BatchFragArgs{a.affs_dev, a.frags_dev, a.max_id_dev, a.labels_dev, a.num_labels_dev, a.id_offset, a.size_dev, a.sums_dev};
  }
  BSMI_HIP(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const bool with_filter = filter_value > 0.0 || min_size > 0;
  hipLaunchKernelGGL(batch_set_frag_kernel, dim3(n_blocks), dim3(64), 0, s, b->tab, call, stats_num, with_filter ? 1 : 0);
  size_t most = (size_t)stats_num * 24 / 16;
  if (with_filter) most = std::max(most, (size_t)b->max_frag_id_cap * 8 / 16);
  batch_fill_launch(b->tab, n_blocks, most, s);
  rc = batch_ws_launch(b->tab, n_blocks, (int)shape[0], (int)shape[1], (int)shape[2], min_seed_distance, s);
  if (rc) return rc;
  batch_post_launch(b->tab, n_blocks, shape, filter_value, min_size, crop_offset, crop_shape, stats_num, s);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_seg_batch_rag_graph_u8(bsmi_seg_batch* b, int n_blocks, const bsmi_batch_graph_args* args, const int64_t shape[3], void* stream) {
  int rc = batch_check(b, n_blocks, args, shape);
  if (rc) return rc;
  BatchGraphCall call{};
  for (int i = 0; i < n_blocks; ++i) {
    const bsmi_batch_graph_args& a = args[i];
    if (!a.affs_dev || !a.frags_dev || !a.edges_dev || !a.sums_dev || !a.pair_counts_dev || !a.counts_dev)
      BSMI_FAIL(BSMI_ERR_INVALID, "null argument (block %d)", i);
    call.a[i] = BatchGraphArgs{a.affs_dev, a.frags_dev, a.edges_dev, a.sums_dev, a.pair_counts_dev, a.counts_dev, a.edge_capacity};
  }
  BSMI_HIP(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(batch_set_graph_kernel, dim3(n_blocks), dim3(64), 0, s, b->tab, call);
  batch_fill_launch(b->tab, n_blocks, (size_t)std::max(b->max_icap, b->max_hcap) * 8 / 16, s);
  batch_graph_launch(b->tab, n_blocks, shape, b->max_hcap, s);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

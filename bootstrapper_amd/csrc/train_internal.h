// What the translation units of the training engine share: the training state of a handle, the records the planner leaves
// for the step, a few host helpers and the launchers one file exports to another.  Not part of the C ABI.  A kernel lives in
// the file that launches it:
//   train.hip          the reference map; begin / end, the state's allocations, the small accessors, the step itself
//                      (bsmi_unet_train_forward_backward as a walk over the plan, bsmi_unet_train_adam_step)
//   train_plan.hip     what begin builds per CONV step: the forward pass's fused split-bf16 launches (make_forward_x3 and their
//                      hook in the forward pass, train_forward_conv_x3), the backward data and the input-gradient launches
//   train_pack.hip     weight / bias / head images packed from the flat parameter buffer: the kernels, the pack jobs
//   train_bwd.hip      the element-wise and reduction kernels of the step (loss, head, ReLU mask + pad + bias gradient, pooling,
//                      upsampling, scatter, f32 <-> split, Adam), one launcher per plan-step type
//   train_wgrad.hip    the four weight-gradient kernel families and the weight gradients of one conv stage
//   train_debug.hip    bsmi_unet_train_debug_* (what the per-launch parity tests read)
//   train_targets.hip  affinity / LSD targets (bsmi_train_*_targets): they take a device, not a handle, and share nothing here
//
// Streams.  The step runs on two streams: the caller's (`s`, the `stream` argument of every entry point) and the weight
// gradients' own (TrainState::wstream; null under BSMI_TRAIN_WSTREAM=0, and then everything below happens on `s` in the order
// given and the events are unused).
//   s        forward pass, gradient clears, loss, every train_bwd.hip launch, the input-gradient launches, Adam, the head images
//            and the forward images the next pass reads first (PACK_FWD_EARLY)
//   wstream  per conv stage: operand packing, weight-gradient launches and their finish kernel (train_wgrad.hip); after Adam:
//            the images of PACK_FWD_LATE, then those of PACK_BWD
// Events (all but the group events exist only with a wstream):
//   ConvBwd::ev_g   s -> wstream.  Recorded once the stage's padded gradient gp (and its bias gradient) is written; the
//                   stage's weight gradients wait for it.  They read gp and forward activations only, so the input gradient of
//                   the same stage and whatever follows on s run beside them.
//   ev_join         wstream -> s.  Recorded after the last weight gradient of a pass; s waits for it before the loss read-back,
//                   so a pass that has returned has every gradient, and the next pass may overwrite gp / pk_g / pk_x.
//   ev_adam         s -> wstream.  The parameters are updated: the side stream may pack from them.
//   ev_fwd_packed   wstream -> s.  The PACK_FWD_LATE images are written; the forward pass waits where it first needs one
//                   (train_forward_conv_x3, fwd_packed_pending).
//   ev_packed       wstream -> s.  The PACK_BWD images are written; the step waits before its backward loop (packed_pending).
//   GradGroup::ev   recorded where a group's gradients are final: on s after a head's backward launch, on the weight gradients'
//                   stream after those of a pass's first stage (its bias gradients precede ev_g, which that stream has waited
//                   for).  bsmi_unet_train_wait_grad_group makes a caller's stream wait for one.
#pragma once
#include "unet_internal.h"

namespace bsmi {

// ---- split-bf16 helper: (a, b) -> packed bf16 pair of the high parts and of what they leave ----
typedef __bf16 wg_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float wg_f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  const wg_bf16x2_t h = __builtin_convertvector(wg_f32x2_t{a, b}, wg_bf16x2_t);
  hi = __builtin_bit_cast(uint32_t, h);
  const float ha = __uint_as_float(hi << 16), hb = __uint_as_float(hi & 0xffff0000u);
  const wg_bf16x2_t l = __builtin_convertvector(wg_f32x2_t{a - ha, b - hb}, wg_bf16x2_t);
  lo = __builtin_bit_cast(uint32_t, l);
}

// ---- records ----

// one unit (8 floats of K) of a packed weight image: dst[(u / 2) * Npad + n][(u % 2) * 8 + kk] =
// src[wbase + n * sn + (c0 + kk) * sc + tap] for n < nreal, c0 + kk < creal; zero elsewhere
struct PackUnit {
  long long wbase;  // float offset into the flat parameter buffer, -1: padding unit
  int sn, sc, tap, c0, creal, pad;
};

struct ParamRef {
  std::string key;
  size_t off = 0, count = 0;
  std::vector<int64_t> shape;
};

// The four parameters of one conv stage (prefix.conv_pass.<2 ci>.{weight,bias}, prefix.residual.0.{weight,bias}) or of a head
// (ci = 0), resolved once at begin (find_stage_params): entries of TrainState::params, whose `off` indexes w, g, gt, m and v.
struct StageParams {
  const ParamRef *w = nullptr, *b = nullptr, *rw = nullptr, *rb = nullptr;
};

struct PackJob {  // one packed weight image that must follow the parameters
  PackUnit* units = nullptr;  // device
  int nunits = 0, Npad = 0, nreal = 0;
  float* dst = nullptr;
  uint32_t *dst_hi = nullptr, *dst_lo = nullptr;  // fused split-bf16 image instead (units of 16 channels)
  int window = 2;  // units of one 32-channel chunk (taps x 2): the thread order of pack_weights_x3_kernel
  bool shadowed = false;  // f32 image of a forward launch that trains in its split-bf16 form (make_forward_x3)
  bool backward = false;  // image of an input-gradient launch: first read in the backward pass (packed on the side stream)
  bool late = false;      // forward image of a wide stage, first read a millisecond into the forward pass (side stream as well)
  // bias image (forward launches only)
  long long b0 = -1, b1 = -1;
  float* bias_dst = nullptr;
};

// which images a run_pack_jobs call rewrites
enum PackSet {
  PACK_ALL,        // every image
  PACK_FWD_EARLY,  // those the forward pass reads first (neither backward nor late)
  PACK_BWD,        // those of the input-gradient launches, first read in the backward pass
  PACK_FWD_LATE,   // the wide stages' forward images
};
// F32_LAZY leaves out the f32 weight image of a forward launch that runs in its split-bf16 form during training
// (PackJob::shadowed); the images are then stale until train_refresh_f32_images, which an f32 inference call on the same
// handle triggers (bsmi_unet_forward, unet_forward.hip) -- the bias images and everything the step itself reads are always current.
enum PackF32 { F32_CURRENT, F32_LAZY };

struct ConvBwd {  // backward data of one CONV plan step
  const PlanStep* st = nullptr;
  StageParams par;       // the stage's parameters
  int P[3] = {0, 0, 0};  // border of the padded gradient
  TDesc gp;              // padded gradient [D + 2P][H + 2P][W + 2P][Cpad]
  void* gps = nullptr;   // the same in the split-bf16 activation layout (input gradients as split-bf16 launches), or null
  void* dsplit = nullptr;  // result of the split-bf16 input-gradient launch before split_to_f32_kernel (null: the launch writes f32 sums itself)
  bool dx3 = false;        // the input gradient is a split-bf16 launch
  bool need_dgrad = false;
  ConvArgs dgrad{};      // implicit-GEMM launch of the input gradient
  TileCfg dtile = TILE_256x32;
  TDesc dcat;            // its output when the pass input is a crop / concat (stage 0), else the previous stage's gradient
  bool scatter = false;
  hipEvent_t ev_g = nullptr;  // the padded gradient is written: the weight-gradient stream may start on this stage
};

// (PlanStep::tx3's type, unet_internal.h)
struct TrainFwdX3 {  // a forward CONV step as a fused split-bf16 launch
  ConvArgs a{};
  TileCfg tile = TILE_256x32;
  int nconv_src = 0;
  const void* src_f32[kMaxConvTensors] = {nullptr, nullptr, nullptr};  // sources to split before the launch (null: a split copy exists)
  void* src_split[kMaxConvTensors] = {nullptr, nullptr, nullptr};
  size_t src_g8[kMaxConvTensors] = {0, 0, 0};
  void* out_split = nullptr;  // the launch's result, turned into the step's f32 output tensor afterwards
  size_t out_g8 = 0;
  bool late = false;          // its weight image is packed on the side stream after an optimizer step (TrainState::ev_fwd_packed)
};

// The training state of a handle (bsmi_unet::train), made by bsmi_unet_train_begin for one input shape.  Everything on the
// device is allocated at begin (talloc, freed with the state) except the four grow-only scratch buffers, which the first steps
// size (grow_buf).  "step" = bsmi_unet_train_forward_backward, "Adam" = bsmi_unet_train_adam_step.
struct TrainState {
  // ---- the plan and what begin derives from it (host; fixed after begin) ----
  int64_t in_shape[3] = {0, 0, 0};
  Plan* plan = nullptr;                // the handle's BSMI_PREC_F32 plan of in_shape; the step walks it forward, then in reverse
  std::vector<ConvBwd> convs;          // indexed like plan->steps (empty entries for other step types)
  std::vector<StageParams> head_par;   // indexed like bsmi_unet::heads
  std::vector<std::unique_ptr<TrainFwdX3>> fwd_x3;  // owners of PlanStep::tx3
  std::map<const void*, void*> split_of;  // f32 activation -> its split copy written by an earlier launch of the forward pass
  std::map<const void*, size_t> fwd_job_of;  // bias image of a forward launch -> index of its pack job
  std::map<void*, TDesc> grad_of;      // activation -> its gradient tensor (grad_tensor)
  std::vector<std::pair<void*, size_t>> zero_list;  // the gradient tensors: cleared by the step before its backward loop
  std::vector<void*> allocs;           // every talloc of the state
  size_t out_vox = 0;

  // ---- parameters: flat f32 buffers in state_dict order, ParamRef::off into each of them ----
  std::vector<ParamRef> params;        // fixed after begin: StageParams points into it
  std::map<std::string, size_t> index; // key -> index into params
  size_t nparams = 0;
  float* w = nullptr;  // parameters.  written: begin (from the handle's host weights), Adam.  read: every pack kernel, end (back to the host)
  float* g = nullptr;  // gradients.  cleared by the step; written by its head / bias / weight-gradient launches (atomics or folds);
                       // read by Adam and by the caller between the two (the data-parallel all-reduce runs on it)
  float *m = nullptr, *v = nullptr;  // Adam moments.  written: Adam, bsmi_unet_train_write_param
  // tap-major workspace of the split-bf16 weight gradients, same offsets as g; null when they run in f32 (BSMI_WGRAD_X3=0 or f32
  // arithmetic).  MUST BE ZERO between steps: wgrad_x3_kernel adds into it, wgrad_finish_kernel moves every non-zero value into
  // g and writes the zero back.  In deterministic mode the launches add into gt_det instead and gt only says "split form".
  float* gt = nullptr;
  int adam_t = 0;

  // ---- packed images (train_pack.hip) ----
  std::vector<PackJob> jobs;           // in launch order: forward f32 images, forward split-bf16 images, input-gradient images
  bool f32_images_stale = false;       // a F32_LAZY pack has run since the shadowed f32 images were last written

  // ---- scratch of the step ----
  float* zero_bias = nullptr;        // [2048] zeros, never written: bias operand of the input-gradient launches
  double* loss_sums = nullptr;       // [4], cleared and reused per head: loss_sums_kernel (or its fold) -> loss_grad_kernel
  double* loss_part = nullptr;       // [512][4] deterministic mode: loss_sums_kernel -> fold_kernel; fully written before it is read
  float* loss_dev = nullptr;         // [1] cleared by the step, loss_grad_kernel adds every head's loss; read back at the end of the step
  std::vector<float*> head_out;      // per head: sigmoid outputs [C][D][H][W] of the last forward pass (the forward pass writes, loss and head backward read)
  std::vector<float*> head_dp;       // per head: dL/dp (loss_grad_kernel writes, head_bwd_kernel reads)
  // Grow-only buffers.  pk_g, pk_x and gt_det belong to the weight gradients' stream, det_part to the caller's.
  //   pk_g, pk_x  packed operands of the split-bf16 weight gradient: wgrad_pack_kernel writes every byte a launch reads (the
  //               all-zero group included), g once per conv stage and x before every launch.  Need not be zero.
  //   gt_det      deterministic mode: per-line-range copies of ONE weight tensor's tap-major workspace.  MUST BE ZERO between the
  //               launches of two weight tensors: a grown buffer is cleared on the stream that uses it, wgrad_finish_det_kernel
  //               writes back a zero for every value it takes.
  //   det_part    deterministic mode: per-workgroup partial sums of head_bwd_kernel / colsum_kernel for fold_kernel.  The
  //               producer writes every row its fold reads.  Need not be zero.
  char *pk_g = nullptr, *pk_x = nullptr;
  size_t pk_g_bytes = 0, pk_x_bytes = 0;
  char *gt_det = nullptr, *det_part = nullptr;
  size_t gt_det_bytes = 0, det_part_bytes = 0;
  std::vector<bsmi_unet_train_step_info> rec;  // what the last pass launched per plan step (bsmi_unet_train_debug_step_info)

  // ---- streams and events (see the top of this file) ----
  hipStream_t wstream = nullptr;     // the weight gradients' own stream (null: BSMI_TRAIN_WSTREAM=0, everything on the caller's)
  bool own_wstream = false;
  bool wstream_wanted = false;       // BSMI_TRAIN_WSTREAM at begin (known before the stream itself is made)
  hipEvent_t ev_join = nullptr;      // its last launch of a backward pass
  hipEvent_t ev_adam = nullptr, ev_packed = nullptr;  // optimizer step done / input-gradient images repacked on the side stream
  hipEvent_t ev_fwd_packed = nullptr;                  // the wide stages' forward images repacked there
  bool packed_pending = false, fwd_packed_pending = false;  // an ev_packed / ev_fwd_packed nobody has waited for yet
  // Gradient groups: the parameters of one ConvPass / head are one contiguous range of the flat buffers (their keys share
  // a prefix and the buffers follow the sorted keys); a group's gradients are final once the backward pass has left its
  // first stage.  group_order: groups in the order the backward pass finishes them; an event per group is recorded on
  // the backward stream so that a data-parallel caller can start reducing a group while the pass goes on.
  struct GradGroup { std::string prefix; size_t off = 0, count = 0; hipEvent_t ev = nullptr; };
  std::vector<GradGroup> groups;       // completion order
  std::map<std::string, int> group_of; // prefix -> index into groups
};

// ---- host helpers ----

// dev knobs: on unless set to something that starts with '0'
static inline bool env_on(const char* name) {
  const char* e = getenv(name);
  return !e || e[0] != '0';
}
// workgroups of 256 threads for n items of a grid-stride kernel, at most `cap`
static inline unsigned grid_1d(size_t n, size_t cap) { return (unsigned)std::min<size_t>((n + 255) / 256, cap); }
static inline size_t tensor_bytes(const TDesc& t) { return (size_t)t.D * t.H * t.W * t.Cpad * sizeof(float); }
// room behind a tensor that the implicit-GEMM kernels' padded tile loads may touch
static inline size_t tensor_slack(const TDesc& t) { return (size_t)8 * t.W * t.Cpad * sizeof(float) + 4096; }
// sum of (k - 1) over the stages of a ConvPass: what the pass crops, and twice the origin of its residual branch
static inline void pass_crop(const PassSite& p, int crop[3]) {
  for (int d = 0; d < 3; ++d) crop[d] = 0;
  for (int i = 0; i < p.nconv; ++i)
    for (int d = 0; d < 3; ++d) crop[d] += p.k[i][d] - 1;
}
// input channels of a ConvPass (its residual's Cin) and of its stage ci
static inline int pass_cin(const PassSite& p) { return p.cin[0] + (p.nslots > 1 ? p.cin[1] : 0); }
static inline int stage_cin(const PassSite& p, int ci) { return ci == 0 ? pass_cin(p) : p.cout; }
// source `sl` of an implicit-GEMM launch: a channels-last tensor of t's geometry at `base` (4 bytes per channel, f32 and split alike)
static inline void set_conv_src(ConvArgs& a, int sl, const TDesc& t, const void* base) {
  const int64_t es = 4;
  a.t[sl].base = (uint64_t)(uintptr_t)base;
  a.t[sl].sz = (int32_t)((int64_t)t.H * t.W * t.Cpad * es);
  a.t[sl].sy = (int32_t)((int64_t)t.W * t.Cpad * es);
  a.t[sl].sx = (int32_t)((int64_t)t.Cpad * es);
}

// ---- train.hip ----
int talloc(TrainState* ts, void** p, size_t bytes, bool zero);  // device memory that lives as long as the state
// a scratch buffer of the training state that only grows (first steps); zero_new: a grown buffer starts as zeros
int grow_buf(hipStream_t s, char** buf, size_t* have, size_t need, bool zero_new);
// begin only: BSMI_ERR_MISSING with the key's name where the state_dict lacks it
int find_param(const TrainState* ts, const std::string& key, const ParamRef** out);
int find_stage_params(const TrainState* ts, const std::string& prefix, int ci, StageParams* out);

// ---- train_plan.hip (begin) ----
int grad_tensor(TrainState* ts, const TDesc& act, TDesc* out);  // gradient tensor of an activation (same geometry, f32), created on first use
int make_forward_x3(TrainState* ts, PlanStep& st);
int make_conv_bwd(bsmi_unet* h, TrainState* ts);  // TrainState::convs, the input-gradient launches included

// ---- train_pack.hip ----
int upload_units(TrainState* ts, const std::vector<PackUnit>& u, PackUnit** dev);
// the units of a planner's unit list (build_entries) as reads of the flat parameter buffer
std::vector<PackUnit> entry_units(const std::vector<PackEntry>& ents, const StageParams& par);
int make_forward_job(TrainState* ts, PassSite& p, int ci);
int run_pack_jobs(TrainState* ts, hipStream_t s, PackSet set, PackF32 f32);
void launch_pack_head(const TrainState* ts, const HeadSite& hd, const StageParams& par, hipStream_t s);

// ---- train_bwd.hip: the launches of the step on the caller's stream, by plan-step type ----
void launch_f32_to_split(const void* src_f32, void* dst_split, size_t ngroups8, hipStream_t s);
void launch_split_to_f32(const void* src_split, void* dst_f32, size_t ngroups8, hipStream_t s);
int launch_loss(TrainState* ts, int head, size_t n, const float* target, const float* weight, bool det, hipStream_t s);
int launch_head_bwd(bsmi_unet* h, const PlanStep& st, bool det, hipStream_t s);
void launch_up_bwd(TrainState* ts, size_t step, bool det, hipStream_t s);
void launch_pool_bwd(TrainState* ts, const PlanStep& st, hipStream_t s);
int launch_mask_pad_bias(TrainState* ts, size_t step, bool det, hipStream_t s);  // g = dY [Y > 0] into gp (and gps), bias gradients
int launch_scatter(TrainState* ts, const ConvBwd& cb, hipStream_t s);            // dcat added into the gradients of the pass's sources
void launch_adam(TrainState* ts, float lr, float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float gscale, hipStream_t s);

// ---- train_wgrad.hip ----
// weight gradients of CONV plan step `step` (and of the pass's residual weight on its last stage) on stream sw
int launch_wgrad_stage(TrainState* ts, size_t step, bool det, hipStream_t sw);

}  // namespace bsmi

// Training step of the U-Net engine: loss, backward pass, Adam, on the device in fp32 (the reference trains
// in fp32: models/3d_affs/train.py, training.py:96-137).
//
// Reference being replaced (paths relative to /root/reference/bootstrapper):
//   models/3d_affs/train.py:152-159   training_step = loss(model(raw), gt, weights); Adam(lr = 0.5e-4)
//   models/3d_affs/model.py:67-92     WeightedMSELoss (masked mean of w (p - t)^2)
//   models/3d_affs/unet.py            autograd of ConvPass / Downsample / Upsample, restated here as explicit kernels
//
// The forward pass is the inference engine's own (bsmi_unet_forward in BSMI_PREC_F32: exact f32 MFMA, every
// activation of the block stays resident), so the backward pass walks the same launch plan in reverse:
//   conv stage  g = dY * [Y > 0] into a zero-bordered tensor; bias gradient = column sums; weight gradient by
//               v_mfma_f32_32x32x2_f32 straight from global memory (g^T x, one kernel tap per workgroup); input
//               gradient = the SAME implicit-GEMM kernel as the forward pass run over the padded g with flipped,
//               transposed weights -- the cropped 1x1x1 residual branch rides along as one more K-step source,
//               exactly as in the forward launch
//   max-pool    gradient routed to the first maximum of each window; trilinear upsample: transposed interpolation
//   head        two 1x1x1 convolutions + sigmoid, fused with the loss gradient
// Parameters, gradients and Adam moments are flat fp32 device buffers in state_dict order (the gradient buffer
// is what the data-parallel all-reduce runs on); after an optimizer step the packed weight images of the
// forward and backward launches are rewritten on the device.
//
// This file: bsmi_unet_train_begin / _end, the state's allocations, the accessors and the two entry points of a step.  The
// rest of the engine is in train_*.hip; train_internal.h has the file map, the training state and the stream rules.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "train_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

// Which convolutions of the step run as split-bf16 launches: all of them under bsmi_unet_train_set_arithmetic(h, 1)
// (the default); BSMI_WGRAD_X3 / BSMI_DGRAD_X3 / BSMI_FWD_X3 = 0 take single ones back to f32 (dev knobs, read at begin).
static bool wgrad_x3_enabled(const bsmi_unet* h) { return h->train_split && env_on("BSMI_WGRAD_X3"); }
static bool fwd_x3_enabled(const bsmi_unet* h) { return h->train_split && env_on("BSMI_FWD_X3") && two_waves_per_simd(); }
// (BSMI_DGRAD_X3: make_conv_bwd)

int talloc(TrainState* ts, void** p, size_t bytes, bool zero) {
  BSMI_HIP(hipMalloc(p, bytes + 256));
  ts->allocs.push_back(*p);
  if (zero) BSMI_HIP(hipMemset(*p, 0, bytes + 256));
  return BSMI_OK;
}

int grow_buf(hipStream_t s, char** buf, size_t* have, size_t need, bool zero_new) {
  if (need <= *have) return BSMI_OK;
  BSMI_HIP(hipStreamSynchronize(s));
  if (*buf) BSMI_HIP(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  BSMI_HIP(hipMalloc((void**)buf, need + 4096));
  // on the stream that uses the buffer: hipMemset runs on the null stream, which a non-blocking stream (the weight gradients' own)
  // does not wait for -- a launch could add into the buffer before the fill had passed (seen: two "deterministic" runs 2 974
  // gradient values apart, once in four test-suite runs)
  if (zero_new) BSMI_HIP(hipMemsetAsync(*buf, 0, need + 4096, s));
  *have = need;
  return BSMI_OK;
}

void free_train_state(bsmi_unet* h) {
  if (!h->train) return;
  TrainState& ts = *h->train;
  if (ts.plan)
    for (PlanStep& st : ts.plan->steps) st.tx3 = nullptr;
  for (auto& g : ts.groups)
    if (g.ev) (void)hipEventDestroy(g.ev);
  for (auto& cb : ts.convs)
    if (cb.ev_g) (void)hipEventDestroy(cb.ev_g);
  for (hipEvent_t ev : {ts.ev_join, ts.ev_adam, ts.ev_packed, ts.ev_fwd_packed})
    if (ev) (void)hipEventDestroy(ev);
  // (wstream is the device's side stream, shared by every training state of the process: not destroyed here)
  if (ts.own_wstream && ts.wstream) (void)hipStreamDestroy(ts.wstream);
  for (void* p : ts.allocs) (void)hipFree(p);
  for (char* p : {ts.pk_g, ts.pk_x, ts.gt_det, ts.det_part})
    if (p) (void)hipFree(p);
  delete h->train;
  h->train = nullptr;
}

int find_param(const TrainState* ts, const std::string& key, const ParamRef** out) {
  auto it = ts->index.find(key);
  if (it == ts->index.end()) BSMI_FAIL(BSMI_ERR_MISSING, "no parameter \"%s\"", key.c_str());
  *out = &ts->params[it->second];
  return BSMI_OK;
}

int find_stage_params(const TrainState* ts, const std::string& prefix, int ci, StageParams* out) {
  const std::string base = prefix + ".conv_pass." + std::to_string(2 * ci);
  int rc;
  if ((rc = find_param(ts, base + ".weight", &out->w)) || (rc = find_param(ts, base + ".bias", &out->b))) return rc;
  if ((rc = find_param(ts, prefix + ".residual.0.weight", &out->rw)) || (rc = find_param(ts, prefix + ".residual.0.bias", &out->rb))) return rc;
  return BSMI_OK;
}

// the gradients of parameter group `prefix` are final at this point of stream s
static int record_group(TrainState* ts, const std::string& prefix, hipStream_t s) {
  BSMI_HIP(hipEventRecord(ts->groups[ts->group_of[prefix]].ev, s));
  return BSMI_OK;
}

// One CONV step of the backward pass, on the caller's stream s and the weight gradients' own.
static int conv_bwd(bsmi_unet* h, size_t step, bool det, hipStream_t s) {
  TrainState* ts = h->train;
  ConvBwd& cb = ts->convs[step];
  const PlanStep& st = *cb.st;
  const PassSite& p = *st.site;
  bsmi_unet_train_step_info& ri = ts->rec[step];
  // 1. g = dY [Y > 0] into the zero-bordered tensor (and its split copy), bias gradients = its column sums
  int rc = launch_mask_pad_bias(ts, step, det, s);
  if (rc) return rc;
  // 2. weight gradients: on their own stream (ts->wstream), beside the input-gradient launch of this stage and whatever the main
  // stream does next -- they only read g (ready: the event below) and forward activations, and write dW.  Many launches of
  // the step have too few tiles for the card; two chains of them side by side fill it better.  BSMI_TRAIN_WSTREAM=0: one stream.
  hipStream_t sw = s;
  if (ts->wstream) {
    sw = ts->wstream;
    BSMI_HIP(hipEventRecord(cb.ev_g, s));
    BSMI_HIP(hipStreamWaitEvent(sw, cb.ev_g, 0));
  }
  if ((rc = launch_wgrad_stage(ts, step, det, sw))) return rc;
  // 3. input gradient: the implicit-GEMM launch, then its sums into the gradients of the pass's sources where they are a crop / concat
  if (cb.need_dgrad) {
    const int prec = cb.dx3 ? BSMI_PREC_BF16X3 : BSMI_PREC_F32;
    if ((rc = launch_conv_igemm(cb.dgrad, prec, cb.dtile, s, h->sk_ws, h->sk_grid))) return rc;
    ri.dgrad = cb.dx3 ? 2 : 1;
    ri.dgrad_raw = cb.dgrad.raw ? 1 : 0;
    ri.dgrad_converted = cb.dsplit ? 1 : 0;
    ri.dgrad_bn = tile_bn(cb.dtile);
    ri.dgrad_ksteps = cb.dgrad.nsteps;
    ri.dgrad_split_k = conv_igemm_split_k(cb.dgrad, prec, cb.dtile, h->sk_grid > 0 ? h->sk_grid : 0) ? 1 : 0;
    ri.dgrad_scatter = cb.scatter ? 1 : 0;
    ri.dgrad_residual = (st.ci == 0 && p.nconv > 1) ? 1 : 0;
    if (cb.dsplit) launch_split_to_f32(cb.dsplit, cb.dcat.ptr, tensor_bytes(cb.dcat) / 32, s);
    if (cb.scatter && (rc = launch_scatter(ts, cb, s))) return rc;
  }
  // the pass's gradients are final when its last weight gradient is (its bias gradients were written before ev_g)
  return st.ci == 0 ? record_group(ts, p.prefix, sw) : BSMI_OK;
}

}  // namespace bsmi

using namespace bsmi;

extern "C" {

int bsmi_unet_train_set_arithmetic(bsmi_unet* h, int split_bf16) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  if (h->train) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_set_arithmetic: call before bsmi_unet_train_begin");
  h->train_split = split_bf16 ? 1 : 0;
  return BSMI_OK;
}

int bsmi_unet_train_set_deterministic(bsmi_unet* h, int on) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  h->train_det = on ? 1 : 0;
  return BSMI_OK;
}

int bsmi_unet_train_begin(bsmi_unet* h, const int64_t in_shape[3]) {
  if (!h || !in_shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (!h->finalized[BSMI_PREC_F32]) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_finalize(BSMI_PREC_F32) first: training runs in fp32");
  BSMI_HIP(hipSetDevice(h->device));
  free_train_state(h);
  std::unique_ptr<TrainState> ts(new TrainState);
  ts->wstream_wanted = env_on("BSMI_TRAIN_WSTREAM");
  for (int d = 0; d < 3; ++d) ts->in_shape[d] = in_shape[d];
  int rc = get_plan(h, BSMI_PREC_F32, in_shape, &ts->plan);
  if (rc) return rc;
  // flat parameter buffer in the order of the weight table (= sorted state_dict keys)
  for (auto& kv : h->weights) {
    ParamRef pr;
    pr.key = kv.first;
    pr.shape = kv.second.shape;
    pr.count = kv.second.data.size();
    pr.off = ts->nparams;
    ts->nparams += (pr.count + 3) / 4 * 4;
    ts->index[pr.key] = ts->params.size();
    ts->params.push_back(pr);
  }
  const size_t pb = ts->nparams * sizeof(float);
  if ((rc = talloc(ts.get(), (void**)&ts->w, pb, true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->g, pb, true))) return rc;
  if (wgrad_x3_enabled(h) && (rc = talloc(ts.get(), (void**)&ts->gt, pb, true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->m, pb, true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->v, pb, true))) return rc;
  for (const ParamRef& pr : ts->params)
    BSMI_HIP(hipMemcpy(ts->w + pr.off, h->weights[pr.key].data.data(), pr.count * sizeof(float), hipMemcpyHostToDevice));
  if ((rc = talloc(ts.get(), (void**)&ts->zero_bias, 2048 * sizeof(float), true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->loss_sums, 4 * sizeof(double), true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->loss_part, 512 * 4 * sizeof(double), true))) return rc;
  if ((rc = talloc(ts.get(), (void**)&ts->loss_dev, sizeof(float), true))) return rc;

  Plan& plan = *ts->plan;
  ts->out_vox = (size_t)plan.out_shape[0] * plan.out_shape[1] * plan.out_shape[2];
  for (const HeadSite& hd : h->heads) {
    StageParams par;
    if ((rc = find_stage_params(ts.get(), hd.prefix, 0, &par))) return rc;
    ts->head_par.push_back(par);
    float *o = nullptr, *dp = nullptr;
    if ((rc = talloc(ts.get(), (void**)&o, ts->out_vox * hd.cout * sizeof(float), true))) return rc;
    if ((rc = talloc(ts.get(), (void**)&dp, ts->out_vox * hd.cout * sizeof(float), true))) return rc;
    ts->head_out.push_back(o);
    ts->head_dp.push_back(dp);
  }
  // forward pack jobs (conv stages, then heads are repacked by pack_head_kernel in the step)
  for (auto* sites : {&h->l_conv, &h->r_conv})
    for (PassSite& p : *sites)
      for (int ci = 0; ci < p.nconv; ++ci)
        if ((rc = make_forward_job(ts.get(), p, ci))) return rc;

  if (fwd_x3_enabled(h))
    for (size_t i = 0; i < plan.steps.size(); ++i) {
      if (plan.steps[i].type != PlanStep::CONV || (plan.fused_first && i < 3)) continue;
      if ((rc = make_forward_x3(ts.get(), plan.steps[i]))) return rc;
    }

  ts->rec.assign(plan.steps.size(), bsmi_unet_train_step_info{});
  if ((rc = make_conv_bwd(h, ts.get()))) return rc;
  // gradient tensors of the remaining activations (pool / upsample / head inputs and outputs)
  for (const PlanStep& st : plan.steps) {
    TDesc t;
    if (st.type == PlanStep::POOL || st.type == PlanStep::UP) {
      if ((rc = grad_tensor(ts.get(), st.in, &t))) return rc;
      if ((rc = grad_tensor(ts.get(), st.out, &t))) return rc;
    } else if (st.type == PlanStep::HEAD) {
      if ((rc = grad_tensor(ts.get(), st.in, &t))) return rc;
    }
  }
  // gradient groups in completion order = the order in which the backward pass (plan steps in reverse) leaves them
  auto add_group = [&](const std::string& prefix) -> int {
    if (ts->group_of.count(prefix)) return BSMI_OK;
    TrainState::GradGroup g;
    g.prefix = prefix;
    size_t lo = (size_t)-1, hi = 0;
    for (const ParamRef& pr : ts->params)
      if (pr.key.compare(0, prefix.size() + 1, prefix + ".") == 0) {
        lo = std::min(lo, pr.off);
        hi = std::max(hi, pr.off + (pr.count + 3) / 4 * 4);
      }
    if (lo == (size_t)-1) BSMI_FAIL(BSMI_ERR_STATE, "training plan: no parameters under %s", prefix.c_str());
    g.off = lo;
    g.count = hi - lo;
    BSMI_HIP(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
    ts->group_of[prefix] = (int)ts->groups.size();
    ts->groups.push_back(g);
    return BSMI_OK;
  };
  for (size_t i = plan.steps.size(); i-- > 0;) {
    const PlanStep& st = plan.steps[i];
    if (st.type == PlanStep::HEAD) { if ((rc = add_group(h->heads[st.head].prefix))) return rc; }
    else if (st.type == PlanStep::CONV && st.ci == 0) { if ((rc = add_group(st.site->prefix))) return rc; }
  }
  {
    size_t covered = 0;
    for (auto& g : ts->groups) covered += g.count;
    if (covered != ts->nparams) BSMI_FAIL(BSMI_ERR_STATE, "training plan: gradient groups cover %zu of %zu parameters", covered, ts->nparams);
  }
  if (ts->wstream_wanted) {
    // ONE side stream per device and process, kept: the runtime has few hardware queues (GPU_MAX_HW_QUEUES), a process that
    // already runs 20 segmentation lanes and two predict lanes shares queues from the next stream on, and a stream per Trainer
    // (bench.py builds four) left later work in the process measurably slower
    static std::mutex mu;
    static hipStream_t side[16] = {nullptr};
    std::lock_guard<std::mutex> lk(mu);
    if (h->device >= 0 && h->device < 16) {
      if (!side[h->device]) BSMI_HIP(hipStreamCreateWithFlags(&side[h->device], hipStreamNonBlocking));
      ts->wstream = side[h->device];
    } else {  // (no such node; a stream of the state's own, destroyed with it)
      BSMI_HIP(hipStreamCreateWithFlags(&ts->wstream, hipStreamNonBlocking));
      ts->own_wstream = true;
    }
    for (hipEvent_t* ev : {&ts->ev_join, &ts->ev_adam, &ts->ev_packed, &ts->ev_fwd_packed}) BSMI_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    for (size_t i = 0; i < ts->convs.size(); ++i)
      if (plan.steps[i].type == PlanStep::CONV) BSMI_HIP(hipEventCreateWithFlags(&ts->convs[i].ev_g, hipEventDisableTiming));
  }
  h->train = ts.release();
  return run_pack_jobs(h->train, nullptr, PACK_ALL, F32_CURRENT) || hipDeviceSynchronize() != hipSuccess ? BSMI_ERR_HIP : BSMI_OK;
}

int bsmi_unet_train_num_params(bsmi_unet* h, uint64_t* count) {
  if (!h || !h->train || !count) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  *count = h->train->nparams;
  return BSMI_OK;
}

int bsmi_unet_train_buffers(bsmi_unet* h, float** params_dev, float** grads_dev) {
  if (!h || !h->train) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  if (params_dev) *params_dev = h->train->w;
  if (grads_dev) *grads_dev = h->train->g;
  return BSMI_OK;
}

int bsmi_unet_train_param_info(bsmi_unet* h, const char* key, uint64_t* offset, uint64_t* count) {
  if (!h || !h->train || !key) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  const ParamRef* pr;
  const int rc = find_param(h->train, key, &pr);
  if (rc) return rc;
  if (offset) *offset = pr->off;
  if (count) *count = pr->count;
  return BSMI_OK;
}

int bsmi_unet_train_forward_backward(bsmi_unet* h, const float* raw_dev, const float* const* targets_dev, const float* const* weights_dev,
                                     float* loss_host, void* stream) {
  if (!h || !h->train || !raw_dev || !targets_dev || !weights_dev) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  TrainState* ts = h->train;
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  Plan& plan = *ts->plan;
  const int nheads = (int)h->heads.size();
  const bool det = h->train_det != 0;
  // forward (the inference engine), sigmoid outputs kept for the loss
  for (size_t i = 0; i < ts->rec.size(); ++i) {
    ts->rec[i] = bsmi_unet_train_step_info{};
    ts->rec[i].type = (int32_t)plan.steps[i].type;
    ts->rec[i].deterministic = det ? 1 : 0;
  }
  h->train_forward = true;  // CONV steps with a split-bf16 form run it (PlanStep::tx3)
  int rc = bsmi_unet_forward(h, BSMI_PREC_F32, raw_dev, BSMI_RAW_F32, ts->in_shape, ts->head_out.data(), nullptr, stream);
  h->train_forward = false;
  if (rc) return rc;
  // clear gradients
  BSMI_HIP(hipMemsetAsync(ts->g, 0, ts->nparams * sizeof(float), s));
  for (auto& z : ts->zero_list) BSMI_HIP(hipMemsetAsync(z.first, 0, z.second, s));
  BSMI_HIP(hipMemsetAsync(ts->loss_dev, 0, sizeof(float), s));
  // loss and dL/dp per head
  for (int hd = 0; hd < nheads; ++hd)
    if ((rc = launch_loss(ts, hd, ts->out_vox * h->heads[hd].cout, targets_dev[hd], weights_dev[hd], det, s))) return rc;
  // backward through the plan
  if (ts->packed_pending) {  // the input-gradient images of the last optimizer step (packed on the side stream)
    BSMI_HIP(hipStreamWaitEvent(s, ts->ev_packed, 0));
    ts->packed_pending = false;
  }
  for (size_t i = plan.steps.size(); i-- > 0 && !rc;) {
    const PlanStep& st = plan.steps[i];
    switch (st.type) {
      case PlanStep::HEAD: rc = launch_head_bwd(h, st, det, s); break;
      case PlanStep::UP: launch_up_bwd(ts, i, det, s); break;
      case PlanStep::POOL: launch_pool_bwd(ts, st, s); break;
      case PlanStep::CONV: rc = conv_bwd(h, i, det, s); break;
      default: break;
    }
  }
  if (rc) return rc;
  BSMI_HIP(hipGetLastError());
  if (ts->wstream) {  // the caller's stream ends the pass after the last weight gradient
    BSMI_HIP(hipEventRecord(ts->ev_join, ts->wstream));
    BSMI_HIP(hipStreamWaitEvent(s, ts->ev_join, 0));
  }
  if (loss_host) {
    BSMI_HIP(hipMemcpyAsync(loss_host, ts->loss_dev, sizeof(float), hipMemcpyDeviceToHost, s));
    BSMI_HIP(hipStreamSynchronize(s));
  }
  return BSMI_OK;
}

int bsmi_unet_train_last_loss(bsmi_unet* h, float* loss_host, void* stream) {
  if (!h || !h->train || !loss_host) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipMemcpyAsync(loss_host, h->train->loss_dev, sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
  BSMI_HIP(hipStreamSynchronize((hipStream_t)stream));
  return BSMI_OK;
}

int bsmi_unet_train_prediction(bsmi_unet* h, int head, float** out_dev, uint64_t* count) {
  if (!h || !h->train || !out_dev) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  if (head < 0 || head >= (int)h->train->head_out.size()) BSMI_FAIL(BSMI_ERR_INVALID, "head %d out of range", head);
  *out_dev = h->train->head_out[head];
  if (count) *count = (uint64_t)h->train->out_vox * h->heads[head].cout;
  return BSMI_OK;
}

int bsmi_unet_train_grad_groups(bsmi_unet* h, int max_n, int* n, uint64_t* offsets, uint64_t* counts) {
  if (!h || !h->train || !n) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  *n = (int)h->train->groups.size();
  for (int i = 0; i < *n && i < max_n; ++i) {
    if (offsets) offsets[i] = h->train->groups[i].off;
    if (counts) counts[i] = h->train->groups[i].count;
  }
  return BSMI_OK;
}

int bsmi_unet_train_wait_grad_group(bsmi_unet* h, int group, void* stream) {
  if (!h || !h->train) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  if (group < 0 || group >= (int)h->train->groups.size()) BSMI_FAIL(BSMI_ERR_INVALID, "gradient group %d out of range", group);
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipStreamWaitEvent((hipStream_t)stream, h->train->groups[group].ev, 0));
  return BSMI_OK;
}

int bsmi_unet_train_write_param(bsmi_unet* h, const char* key, int what, const float* host_in) {
  if (!h || !h->train || !key || !host_in) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  if (what != 2 && what != 3) BSMI_FAIL(BSMI_ERR_INVALID, "only the Adam moments (2, 3) can be written; parameters go through bsmi_unet_load_weight");
  const ParamRef* found;
  const int rc = find_param(h->train, key, &found);
  if (rc) return rc;
  const ParamRef& pr = *found;
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipDeviceSynchronize());
  BSMI_HIP(hipMemcpy((what == 2 ? h->train->m : h->train->v) + pr.off, host_in, pr.count * sizeof(float), hipMemcpyHostToDevice));
  return BSMI_OK;
}

int bsmi_unet_train_step_count(bsmi_unet* h, int set_to, int* value) {
  if (!h || !h->train) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  if (set_to >= 0) h->train->adam_t = set_to;
  if (value) *value = h->train->adam_t;
  return BSMI_OK;
}

int bsmi_unet_train_adam_step(bsmi_unet* h, float lr, float beta1, float beta2, float eps, float grad_scale, void* stream) {
  if (!h || !h->train) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called");
  TrainState* ts = h->train;
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  ts->adam_t += 1;
  const float bc1 = 1.f - powf(beta1, (float)ts->adam_t);
  const float bc2 = 1.f - powf(beta2, (float)ts->adam_t);
  launch_adam(ts, lr, beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale, s);
  int rc;
  if (ts->wstream) {
    // the images of the input-gradient launches are first read in the NEXT backward pass: they are packed on the side stream,
    // beside the forward images here and the forward pass that follows (bsmi_unet_train_forward_backward waits for ev_packed
    // before its backward pass)
    BSMI_HIP(hipEventRecord(ts->ev_adam, s));
    BSMI_HIP(hipStreamWaitEvent(ts->wstream, ts->ev_adam, 0));
    if ((rc = run_pack_jobs(ts, ts->wstream, PACK_FWD_LATE, F32_LAZY))) return rc;
    BSMI_HIP(hipEventRecord(ts->ev_fwd_packed, ts->wstream));
    ts->fwd_packed_pending = true;
    if ((rc = run_pack_jobs(ts, ts->wstream, PACK_BWD, F32_LAZY))) return rc;
    BSMI_HIP(hipEventRecord(ts->ev_packed, ts->wstream));
    ts->packed_pending = true;
    rc = run_pack_jobs(ts, s, PACK_FWD_EARLY, F32_LAZY);
  } else {
    rc = run_pack_jobs(ts, s, PACK_ALL, F32_LAZY);
  }
  if (rc) return rc;
  for (size_t i = 0; i < h->heads.size(); ++i) launch_pack_head(ts, h->heads[i], ts->head_par[i], s);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

int bsmi_unet_train_read_param(bsmi_unet* h, const char* key, int what, float* host_out) {
  if (!h || !h->train || !key || !host_out) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  const ParamRef* found;
  const int rc = find_param(h->train, key, &found);
  if (rc) return rc;
  const ParamRef& pr = *found;
  const float* src = what == 0 ? h->train->w : (what == 1 ? h->train->g : (what == 2 ? h->train->m : h->train->v));
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipDeviceSynchronize());
  BSMI_HIP(hipMemcpy(host_out, src + pr.off, pr.count * sizeof(float), hipMemcpyDeviceToHost));
  return BSMI_OK;
}

int bsmi_unet_train_end(bsmi_unet* h) {
  if (h && h->train) {
    // the trained parameters become the handle's weights: host copies refreshed, the bf16 images re-packed on demand
    BSMI_HIP(hipSetDevice(h->device));
    BSMI_HIP(hipDeviceSynchronize());
    const int rrc = train_refresh_f32_images(h, nullptr);  // the f32 images stay the handle's: not left stale
    if (rrc) return rrc;
    BSMI_HIP(hipDeviceSynchronize());
    for (const ParamRef& pr : h->train->params)
      BSMI_HIP(hipMemcpy(h->weights[pr.key].data.data(), h->train->w + pr.off, pr.count * sizeof(float), hipMemcpyDeviceToHost));
    for (auto* sites : {&h->l_conv, &h->r_conv})
      for (PassSite& p : *sites)
        for (int ci = 0; ci < p.nconv; ++ci)
          for (int prec : {BSMI_PREC_BF16, BSMI_PREC_BF16X3}) {
            PackedConv& pc = p.packed[prec][ci];
            if (pc.w) (void)hipFree(pc.w);
            if (pc.bias) (void)hipFree(pc.bias);
            pc = PackedConv();
          }
    h->finalized[BSMI_PREC_BF16] = false;
    h->finalized[BSMI_PREC_BF16X3] = false;
  }
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipDeviceSynchronize());
  free_train_state(h);
  return BSMI_OK;
}

}  // extern "C"

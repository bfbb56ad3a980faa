// The forward pass of the U-Net engine: bsmi_unet_forward walks the cached plan of (precision, input shape) and queues its
// launches on the caller's stream; around it the stream-K workspace set-up, the opt-in forward chain and the per-step profiling
// events with their bsmi_unet_profile_* entry points.
#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "unet_internal.h"
#include "unet_ops.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

// Wait for the events of the profiled forwards of `plan` that have not been read yet and fold them into the totals.
static int harvest(bsmi_unet* h, Plan* plan) {
  if (!plan || plan->inflight.empty()) return BSMI_OK;
  const size_t n = plan->steps.size();
  for (auto& set : plan->inflight) {
    plan->last_ms.assign(n, 0.f);
    BSMI_HIP(hipEventSynchronize(set[2 * n - 1]));
    for (size_t i = 0; i < n; ++i) {
      float t = 0.f;
      BSMI_HIP(hipEventElapsedTime(&t, set[2 * i], set[2 * i + 1]));
      plan->last_ms[i] = t;
      // with the fused first pass, steps 0 and 1 launch nothing: their work is done (and timed) in step 2
      const int ty = (plan->fused_first && i < 2) ? (int)PlanStep::CONV : (int)plan->steps[i].type;
      h->prof_ms[ty] += t;
      h->prof_flops[ty] += plan->steps[i].flops;
      if (ty == 1) h->prof_exec += plan->steps[i].exec_flops > 0 ? plan->steps[i].exec_flops : plan->steps[i].flops * (plan->prec == BSMI_PREC_BF16X3 ? 3.0 : 1.0);
      h->prof_launches[ty] += ((plan->fused_first && i < 2) || plan->steps[i].pool_fused) ? 0 : 1;
    }
    plan->spare.push_back(std::move(set));
  }
  plan->inflight.clear();
  plan->pending = false;
  return BSMI_OK;
}

// Opt-in (BSMI_FORWARD_CHAIN=1): one forward pass in flight per GPU and process.  Round 4 found predictions corrupted when two
// forward passes overlapped on one GPU (two handles on two streams, or two processes): the victim was the head kernel, the only
// launch of a pass with a scratch segment (272 bytes per lane); every other launch's output was intact.  The
// head kernel keeps its channels in registers now and no kernel of the engine has a scratch segment (tests/test_kernel_resources.py),
// so passes may overlap.  The chain stays as a diagnostic: a forward on another stream than the previous one first waits, on the
// device, for that one's last launch (an event recorded at the end of every forward).
namespace {
std::mutex g_chain_mu;
struct ChainState { hipEvent_t done = nullptr; hipStream_t last = nullptr; bool any = false; };
ChainState g_chain[16];
}  // namespace
struct ForwardChain {
  std::unique_lock<std::mutex> lock{g_chain_mu};
};
static bool forward_chain_on() {   // BSMI_FORWARD_CHAIN=1: on.  Off by default since the head kernel lost its scratch segment (the trigger)
  static const bool on = [] { const char* e = getenv("BSMI_FORWARD_CHAIN"); return e && e[0] == '1'; }();
  return on;
}
static int forward_chain_enter(int device, hipStream_t s) {
  if (device < 0 || device >= 16 || !forward_chain_on()) return BSMI_OK;
  ChainState& c = g_chain[device];
  if (c.any && c.last != s) BSMI_HIP(hipStreamWaitEvent(s, c.done, 0));
  return BSMI_OK;
}
static int forward_chain_leave(int device, hipStream_t s) {
  if (device < 0 || device >= 16 || !forward_chain_on()) return BSMI_OK;
  ChainState& c = g_chain[device];
  if (!c.done) BSMI_HIP(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
  BSMI_HIP(hipEventRecord(c.done, s));
  c.last = s;
  c.any = true;
  return BSMI_OK;
}

}  // namespace bsmi

extern "C" {

int bsmi_unet_forward(bsmi_unet* h, int precision, const void* raw_dev, int raw_dtype,
                      const int64_t in_shape[3], float* const* out_f32_dev,
                      uint8_t* const* out_u8_dev, void* stream) {
  if (!h || !raw_dev || !in_shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (precision < 0 || precision >= BSMI_NUM_PREC) BSMI_FAIL(BSMI_ERR_INVALID, "unknown precision %d", precision);
  if (raw_dtype != BSMI_RAW_U8 && raw_dtype != BSMI_RAW_F32 && raw_dtype != BSMI_RAW_U8_UNIT) BSMI_FAIL(BSMI_ERR_INVALID, "unknown raw dtype %d", raw_dtype);
  if (!h->finalized[precision]) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_finalize(precision=%d) has not been called", precision);
  int rc = check_shape_arg(in_shape);
  if (rc) return rc;
  BSMI_HIP(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  ForwardChain chain_guard;   // (holds the process-wide lock of the chain until the launches are queued)
  if ((rc = forward_chain_enter(h->device, s))) return rc;
  Plan* plan_ptr = nullptr;
  rc = get_plan(h, precision, in_shape, &plan_ptr);
  if (rc) return rc;
  Plan& plan = *plan_ptr;
  h->last_plan = &plan;
  // profile_period N > 0: every Nth forward records its per-step events (N = 1: every forward)
  const bool prof = h->profile_period > 0 && (h->profile_count++ % h->profile_period) == 0;
  if (prof || h->profile_period == 0) plan.profiled = prof;
  if (prof) plan.pending = true;
  if (prof) {
    // a fresh set of events for this forward: recording must not wait for an earlier forward to finish (the caller may
    // have many blocks in flight); bsmi_unet_profile_read / _totals read the sets
    const size_t n_ev = 2 * plan.steps.size();
    if (plan.inflight.size() >= 4096) {  // nobody reads: do not grow without bound
      rc = harvest(h, &plan);
      if (rc) return rc;
    }
    if (!plan.spare.empty() && plan.spare.back().size() == n_ev) {
      plan.events = std::move(plan.spare.back());
      plan.spare.pop_back();
    } else {
      plan.events.assign(n_ev, nullptr);
      for (auto& e : plan.events) BSMI_HIP(hipEventCreate(&e));
    }
  }
  if (!h->sk_grid) {
    const char* e = getenv("BSMI_STREAMK");
    if ((e && e[0] == '0') || h->sk_request == 0) {
      h->sk_grid = -1;
    } else {
      hipDeviceProp_t prop;
      BSMI_HIP(hipGetDeviceProperties(&prop, h->device));
      h->sk_grid = h->sk_request >= 0 ? h->sk_request : prop.multiProcessorCount / 8 * 8;
      if (const char* g = getenv("BSMI_SK_GRID")) h->sk_grid = std::max(8, atoi(g) / 8 * 8);  // tests: force cuts on small nets
      BSMI_HIP(hipMalloc((void**)&h->sk_ws, stream_k_ws_bytes(h->sk_grid)));
      // (on the forward's own stream: a fill on the null stream is not ordered before launches on a non-blocking stream)
      BSMI_HIP(hipMemsetAsync((char*)h->sk_ws + stream_k_ws_bytes(h->sk_grid) - 64, 0, 64, s));
    }
  }
  // f32 inference on a handle that is training: the f32 images of the launches that train in their split-bf16 form are
  // brought up to date first (train_pack.hip keeps only what the training step itself reads current)
  if (h->train && precision == BSMI_PREC_F32 && !h->train_forward && (rc = train_refresh_f32_images(h, s))) return rc;
  size_t step_idx = 0;
  for (const PlanStep& st : plan.steps) {
    if (prof) BSMI_HIP(hipEventRecord(plan.events[2 * step_idx], s));
    if (plan.fused_first && step_idx < 3) {
      // l_conv.0 as one launch in place of its second conv; the input-preparation and first-conv steps fall away
      if (step_idx == 2) {
        FirstPassArgs fa;
        fa.raw = raw_dev; fa.raw_dtype = raw_dtype;
        fa.D = plan.steps[0].out.D; fa.H = plan.steps[0].out.H; fa.W = plan.steps[0].out.W;
        fa.out = (uint16_t*)st.out.ptr;
        const FirstPassWeights& fw = precision == BSMI_PREC_BF16X3 ? h->first_pass_x3 : h->first_pass;
        fa.w1a = fw.w1a; fa.w2a = fw.w2a; fa.vec = fw.vec;
        fa.split = fw.split;
        rc = launch_first_pass(fa, h->sk_grid > 0 ? h->sk_grid : 256, s);
        if (rc) return rc;
      }
      if (prof) BSMI_HIP(hipEventRecord(plan.events[2 * step_idx + 1], s));
      ++step_idx;
      continue;
    }
    switch (st.type) {
      case PlanStep::INPUT:
        rc = launch_input_prep(precision, raw_dev, raw_dtype, st.out.ptr, st.out.C, st.out.Cpad,
                               (size_t)st.out.D * st.out.H * st.out.W, s);
        break;
      case PlanStep::CONV:
        if (st.use_wino && !(st.tx3 && h->train_forward)) {
          if ((rc = launch_wino_in(st.wino_in, s))) break;
          if ((rc = launch_conv_igemm(st.wino_gemm, precision, st.tile, s, h->sk_ws, h->sk_grid))) break;
          if (st.wino_has_res && (rc = launch_conv_igemm(st.wino_res, precision, st.tile, s, h->sk_ws, h->sk_grid))) break;
          if (st.wino_has_res_low && (rc = launch_conv_igemm(st.wino_res_low, precision, st.tile, s, h->sk_ws, h->sk_grid))) break;
          if (st.wino_has_below && (rc = launch_conv_igemm(st.wino_below, precision, st.below_tile, s, h->sk_ws, h->sk_grid))) break;
          rc = launch_wino_out(st.wino_out, s);
          break;
        }
        rc = (st.tx3 && h->train_forward) ? train_forward_conv_x3(h, st, s)
             : st.use_h16 ? launch_conv_h16(st.h16, st.h16_rows, s)
             : st.use_box ? launch_conv_box(st.box, s)
             : st.use_rh ? launch_conv_rh(st.rh, precision, st.tile, s, h->sk_ws, h->sk_grid)
                         : launch_conv_igemm(st.conv, precision, st.tile, s, h->sk_ws, h->sk_grid);
        break;
      case PlanStep::POOL:
        if (st.pool_fused) break;  // stored by the output transform of the stage before (Planner::rec, fused pooling)
        rc = launch_maxpool(precision, st.in.ptr, st.out.ptr, st.in.D, st.in.H, st.in.W, st.in.Cpad,
                            st.f[0], st.f[1], st.f[2], s);
        break;
      case PlanStep::UP:
        if (st.skip) break;  // its readers interpolate on the fly (Planner::rec, fused upsampling)
        rc = launch_upsample_crop(precision, st.in.ptr, st.out.ptr, st.in.D, st.in.H, st.in.W, st.in.Cpad,
                                  st.out.D, st.out.H, st.out.W, st.f[0], st.f[1], st.f[2], st.o[0], st.o[1], st.o[2], s);
        break;
      case PlanStep::HEAD: {
        const HeadSite& hd = h->heads[st.head];
        float* of = out_f32_dev ? out_f32_dev[st.head] : nullptr;
        uint8_t* ou = out_u8_dev ? out_u8_dev[st.head] : nullptr;
        if (of || ou)
          rc = launch_head(precision, st.in.ptr, st.in.Cpad, hd.cin, hd.cout, hd.hw, hd.hb, of, ou,
                           (size_t)st.in.D * st.in.H * st.in.W, s);
        break;
      }
    }
    if (rc) return rc;
    if (prof) BSMI_HIP(hipEventRecord(plan.events[2 * step_idx + 1], s));
    ++step_idx;
  }
  if (prof) plan.inflight.push_back(std::move(plan.events));
  return forward_chain_leave(h->device, s);
}

int bsmi_unet_profile_enable(bsmi_unet* h, int on) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  h->profile_period = on > 0 ? on : 0;
  h->profile_count = 0;
  return BSMI_OK;
}

int bsmi_unet_profile_read(bsmi_unet* h, int max_n, int* n, int32_t* types, double* ms, double* flops) {
  if (!h || !n) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Plan* plan = h->last_plan;
  if (!plan || !plan->profiled) BSMI_FAIL(BSMI_ERR_STATE, "no profiled forward to read");
  int rc = harvest(h, plan);
  if (rc) return rc;
  const int cnt = (int)plan->steps.size();
  *n = cnt;
  for (int i = 0; i < cnt && i < max_n; ++i) {
    if (types) types[i] = (int32_t)plan->steps[i].type;
    if (ms) ms[i] = plan->last_ms[i];
    if (flops) flops[i] = plan->steps[i].flops;
  }
  return BSMI_OK;
}

int bsmi_unet_profile_totals(bsmi_unet* h, double ms_by_type[5], double flops_by_type[5],
                             int64_t launches_by_type[5], int reset) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  int rc = harvest(h, h->last_plan);
  if (rc) return rc;
  for (int i = 0; i < 5; ++i) {
    if (ms_by_type) ms_by_type[i] = h->prof_ms[i];
    if (flops_by_type) flops_by_type[i] = h->prof_flops[i];
    if (launches_by_type) launches_by_type[i] = h->prof_launches[i];
    if (reset) { h->prof_ms[i] = 0; h->prof_flops[i] = 0; h->prof_launches[i] = 0; }
  }
  return BSMI_OK;
}

int bsmi_unet_profile_executed(bsmi_unet* h, double* executed_flops, int reset) {
  if (!h || !executed_flops) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  *executed_flops = h->prof_exec;
  if (reset) h->prof_exec = 0;
  return BSMI_OK;
}

}  // extern "C"

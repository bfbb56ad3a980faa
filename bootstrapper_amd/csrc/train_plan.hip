// Training engine: what bsmi_unet_train_begin builds per CONV step of the plan (train_internal.h has the file map).
//   make_forward_x3        the step's forward launch once more as a fused split-bf16 launch (PlanStep::tx3), and
//   train_forward_conv_x3  the hook by which the forward pass of a training step runs it
//   make_conv_bwd          TrainState::convs: border and padded gradient of every stage, then
//   make_dgrad             its input-gradient launch: the forward pass's implicit-GEMM kernel over the padded gradient with
//                          flipped, transposed weights
// Each launch gets a PackJob (train_pack.hip) that rewrites its weight image after every optimizer step.
#include <cstdlib>
#include <cstring>

#include "train_internal.h"

namespace bsmi {

int grad_tensor(TrainState* ts, const TDesc& act, TDesc* out) {
  auto it = ts->grad_of.find(act.ptr);
  if (it != ts->grad_of.end()) {
    *out = it->second;
    return BSMI_OK;
  }
  TDesc g = act;
  int rc = talloc(ts, &g.ptr, tensor_bytes(act) + tensor_slack(act), true);
  if (rc) return rc;
  ts->grad_of[act.ptr] = g;
  ts->zero_list.push_back({g.ptr, tensor_bytes(act)});
  *out = g;
  return BSMI_OK;
}

// The forward launch of a gather-form CONV step once more as a fused split-bf16 launch (conv_igemm.hip conv_x3_body): the
// same unit list at 16 channels per unit, K-steps over split copies of the sources (4 bytes per channel like the f32
// tensors: the strides and offsets are the f32 plan's), hi / lo weight images repacked from the parameters every step,
// the bias image of the f32 launch.  The result lands in a split tensor -- the next convolution's source as it is -- and
// is converted to the step's f32 output, which everything else (pooling, upsampling, the backward pass) reads.
int make_forward_x3(TrainState* ts, PlanStep& st) {
  if (st.use_box) return BSMI_OK;  // (forms of the other precisions; an f32 raster-halo step has its gather form in st.conv too)
  PassSite& p = *st.site;
  const int ci = st.ci;
  const PackedConv& pf = p.packed[BSMI_PREC_F32][ci];
  std::vector<PackEntry> ents;
  build_entries(p, ci, BSMI_PREC_BF16X3, ents);
  StageParams par;
  int rc = find_stage_params(ts, p.prefix, ci, &par);
  if (rc) return rc;
  const std::vector<PackUnit> units = entry_units(ents, par);
  const int ntap = (int)(par.w->shape[2] * par.w->shape[3] * par.w->shape[4]);
  const size_t nsteps = ents.size() / kUnitsPerStep;
  std::vector<KStep> ks(nsteps);
  const int64_t es = 4;
  for (size_t s = 0; s < nsteps; ++s) {
    const int slot = ents[kUnitsPerStep * s].slot;
    const TDesc& t = st.slots[slot];
    KStep k;
    memset(&k, 0, sizeof k);
    k.tensor = slot;
    for (int j = 0; j < kUnitsPerStep; ++j) {
      const PackEntry& e = ents[kUnitsPerStep * s + j];
      if (e.dummy) continue;
      const int64_t off = ((((int64_t)(e.dz + st.so[slot][0]) * t.H) + (e.dy + st.so[slot][1])) * t.W + (e.dx + st.so[slot][2])) * t.Cpad + e.c0;
      k.delta[j] = (int32_t)(off * es);
    }
    ks[s] = k;
  }
  std::unique_ptr<TrainFwdX3> fx(new TrainFwdX3());
  fx->tile = pf.tile;
  const size_t wimg = (nsteps * (size_t)pf.Npad + kWeightRowSlack) * kStepRowBytes;
  char* wdev = nullptr;
  if ((rc = talloc(ts, (void**)&wdev, 2 * wimg, true))) return rc;
  KStep* dks = nullptr;
  if ((rc = talloc(ts, (void**)&dks, ks.size() * sizeof(KStep), false))) return rc;
  BSMI_HIP(hipMemcpy(dks, ks.data(), ks.size() * sizeof(KStep), hipMemcpyHostToDevice));
  PackJob job;
  if ((rc = upload_units(ts, units, &job.units))) return rc;
  job.nunits = (int)units.size();
  job.Npad = pf.Npad;
  job.nreal = p.cout;
  job.dst = (float*)wdev;
  job.dst_hi = (uint32_t*)wdev;
  job.dst_lo = (uint32_t*)(wdev + wimg);
  job.window = kUnitsPerStep * ntap;
  // the wide stages' images (2.4 M weights and more: 0.5 of the 0.6 ms of forward packing) are not read before the forward pass
  // has done its first, narrow stages: packed on the side stream, the forward pass waits for them where it first needs one
  job.late = ts->wstream_wanted && (size_t)job.nunits * job.Npad * 16 >= ((size_t)2 << 20);
  fx->late = job.late;
  ts->jobs.push_back(job);
  ConvArgs& a = fx->a;
  memset(&a, 0, sizeof a);
  for (int sl = 0; sl < kMaxConvTensors; ++sl) {
    const int q = sl < st.nsl ? sl : 0;
    const TDesc& t = st.slots[q];
    void* sp = nullptr;
    if (sl < st.nsl) {
      auto it = ts->split_of.find(t.ptr);
      if (it != ts->split_of.end()) {
        sp = it->second;
      } else {
        if ((rc = talloc(ts, &sp, tensor_bytes(t) + tensor_slack(t), true))) return rc;
        fx->src_f32[sl] = t.ptr;
        fx->src_g8[sl] = tensor_bytes(t) / 32;
        ts->split_of[t.ptr] = sp;  // a later launch of the same source (the residual's) finds it split already
      }
      fx->src_split[sl] = sp;
    } else {
      sp = fx->src_split[0];
    }
    set_conv_src(a, sl, t, sp);
  }
  fx->nconv_src = st.nsl;
  if ((rc = talloc(ts, &fx->out_split, tensor_bytes(st.out) + tensor_slack(st.out), true))) return rc;
  fx->out_g8 = tensor_bytes(st.out) / 32;
  ts->split_of[st.out.ptr] = fx->out_split;
  a.steps = dks;
  a.nsteps = (int)ks.size();
  a.w = wdev;
  a.w_lo = wdev + wimg;
  a.bias = pf.bias;
  a.out = fx->out_split;
  a.Do = st.out.D; a.Ho = st.out.H; a.Wo = st.out.W; a.Co = st.out.Cpad;
  a.M = st.out.D * st.out.H * st.out.W;
  a.Npad = pf.Npad;
  a.relu = 1;
  st.tx3 = fx.get();
  ts->fwd_x3.push_back(std::move(fx));
  auto fj = ts->fwd_job_of.find(pf.bias);
  if (fj != ts->fwd_job_of.end()) ts->jobs[fj->second].shadowed = true;
  return BSMI_OK;
}

int train_forward_conv_x3(bsmi_unet* h, const PlanStep& st, hipStream_t s) {
  const TrainFwdX3& fx = *st.tx3;
  if (h->train && h->train->plan) {  // (a step of the training plan: located by address only after it is known to lie inside it)
    const std::vector<PlanStep>& steps = h->train->plan->steps;
    const uintptr_t p0 = (uintptr_t)steps.data(), p1 = (uintptr_t)(steps.data() + steps.size()), ps = (uintptr_t)&st;
    if (ps >= p0 && ps < p1 && steps.size() == h->train->rec.size()) h->train->rec[(ps - p0) / sizeof(PlanStep)].fwd_split = 1;
  }
  if (fx.late && h->train && h->train->fwd_packed_pending) {  // the first wide stage after an optimizer step: its image comes from the side stream
    BSMI_HIP(hipStreamWaitEvent(s, h->train->ev_fwd_packed, 0));
    h->train->fwd_packed_pending = false;
  }
  for (int sl = 0; sl < fx.nconv_src; ++sl)
    if (fx.src_f32[sl]) launch_f32_to_split(fx.src_f32[sl], fx.src_split[sl], fx.src_g8[sl], s);
  const int rc = launch_conv_igemm(fx.a, BSMI_PREC_BF16X3, fx.tile, s, h->sk_ws, h->sk_grid);
  if (rc) return rc;
  launch_split_to_f32(fx.out_split, st.out.ptr, fx.out_g8, s);
  return BSMI_OK;
}

// input-gradient launch of conv stage `ci` of pass p (see the header of train.hip).  For ci >= 1 the output is the gradient
// of the previous stage's activation; for ci == 0 it is `dcat`, the gradient of the (cropped, concatenated) pass input.
static int make_dgrad(TrainState* ts, ConvBwd& cb, const ConvBwd* last_cb) {
  const PlanStep& st = *cb.st;
  PassSite& p = *st.site;
  const int ci = st.ci, n = p.nconv;
  const int* k = p.k[ci];
  const int ntap = k[0] * k[1] * k[2];
  const int cin_total = stage_cin(p, ci);
  const bool x3 = cb.gps != nullptr;  // split-bf16 launch: units of 16 channels, K-steps of 32
  const int SUB = x3 ? 16 : 8;
  const size_t wm = cb.par.w->off, wr = cb.par.rw->off;
  int crop[3];
  pass_crop(p, crop);
  const bool with_res = ci == 0 && n > 1;  // the residual 1x1x1 reads the pass input, whose gradient this launch produces
  const int cpad_g = cb.gp.Cpad;

  std::vector<PackUnit> units;
  std::vector<KStep> steps;
  PackUnit pad_unit{};
  pad_unit.wbase = -1;
  auto close_step = [&]() {
    while (units.size() % kUnitsPerStep) units.push_back(pad_unit);
  };
  // source 0: this stage's padded gradient, all taps; the weight tap is the mirrored one
  const int64_t es = 4;
  const TDesc& g0 = cb.gp;
  for (int c16 = 0; c16 < cpad_g; c16 += kUnitsPerStep * SUB)
    for (int z = 0; z < k[0]; ++z)
      for (int y = 0; y < k[1]; ++y)
        for (int x = 0; x < k[2]; ++x) {
          KStep ks{};
          ks.tensor = 0;
          int j = 0;
          for (int c0 = c16; c0 < std::min(cpad_g, c16 + kUnitsPerStep * SUB); c0 += SUB, ++j) {
            PackUnit pu{};
            pu.wbase = (long long)wm;
            pu.sn = ntap;                       // n of the launch = input channel of the weight
            pu.sc = cin_total * ntap;           // K channel = output channel of the weight
            pu.tap = ((k[0] - 1 - z) * k[1] + (k[1] - 1 - y)) * k[2] + (k[2] - 1 - x);
            pu.c0 = c0;
            pu.creal = p.cout;
            units.push_back(pu);
            const int oz = cb.P[0] - (k[0] - 1) + z, oy = cb.P[1] - (k[1] - 1) + y, ox = cb.P[2] - (k[2] - 1) + x;
            ks.delta[j] = (int32_t)(((((int64_t)oz * g0.H + oy) * g0.W + ox) * g0.Cpad + c0) * es);
          }
          close_step();
          steps.push_back(ks);
        }
  if (with_res) {
    const TDesc& gl = last_cb->gp;
    for (int c16 = 0; c16 < gl.Cpad; c16 += kUnitsPerStep * SUB) {
      KStep ks{};
      ks.tensor = 1;
      int j = 0;
      for (int c0 = c16; c0 < std::min(gl.Cpad, c16 + kUnitsPerStep * SUB); c0 += SUB, ++j) {
        PackUnit pu{};
        pu.wbase = (long long)wr;
        pu.sn = 1;
        pu.sc = cin_total;
        pu.tap = 0;
        pu.c0 = c0;
        pu.creal = p.cout;
        units.push_back(pu);
        const int oz = last_cb->P[0] - crop[0] / 2, oy = last_cb->P[1] - crop[1] / 2, ox = last_cb->P[2] - crop[2] / 2;
        ks.delta[j] = (int32_t)(((((int64_t)oz * gl.H + oy) * gl.W + ox) * gl.Cpad + c0) * es);
      }
      close_step();
      steps.push_back(ks);
    }
  }
  if (steps.size() % 2) {  // even number of K-steps (conv_igemm.hip)
    units.insert(units.end(), kUnitsPerStep, pad_unit);
    steps.push_back(KStep{});
  }
  cb.dtile = choose_tile(cin_total);
  const int Npad = round_up(cin_total, tile_bn(cb.dtile));
  // output tensor
  TDesc out;
  out.C = cin_total;
  out.Cpad = round_up(cin_total, kChanPad);
  out.D = st.out.D + k[0] - 1;
  out.H = st.out.H + k[1] - 1;
  out.W = st.out.W + k[2] - 1;
  int rc;
  if (ci == 0) {
    rc = talloc(ts, &out.ptr, tensor_bytes(out), true);
    if (rc) return rc;
    cb.scatter = true;
  } else {
    // previous stage's activation is slot 0 of this launch
    rc = grad_tensor(ts, st.slots[0], &out);
    if (rc) return rc;
  }
  cb.dcat = out;
  // packed weights + K-steps on the device
  float* wdev = nullptr;  // f32: rows of 16 floats; split-bf16: rows of 32 bf16, hi image then lo image (the same 64 bytes per row)
  const size_t wimg = (steps.size() * (size_t)Npad + kWeightRowSlack) * 16 * sizeof(float);
  rc = talloc(ts, (void**)&wdev, wimg * (x3 ? 2 : 1), true);
  if (rc) return rc;
  KStep* dks = nullptr;
  rc = talloc(ts, (void**)&dks, steps.size() * sizeof(KStep), false);
  if (rc) return rc;
  BSMI_HIP(hipMemcpy(dks, steps.data(), steps.size() * sizeof(KStep), hipMemcpyHostToDevice));
  PackJob job;
  rc = upload_units(ts, units, &job.units);
  if (rc) return rc;
  job.nunits = (int)units.size();
  job.Npad = Npad;
  job.nreal = cin_total;
  job.dst = wdev;
  if (x3) {
    job.dst_hi = (uint32_t*)wdev;
    job.dst_lo = (uint32_t*)((char*)wdev + wimg);
    job.window = kUnitsPerStep * ntap;
  }
  job.backward = true;
  ts->jobs.push_back(job);
  if (Npad > 2048) BSMI_FAIL(BSMI_ERR_INVALID, "dgrad launch wider than the zero-bias buffer");
  if (x3 && with_res && !last_cb->gps) BSMI_FAIL(BSMI_ERR_STATE, "training plan: the residual source has no split copy");
  ConvArgs& a = cb.dgrad;
  memset(&a, 0, sizeof a);
  const TDesc* srcs[kMaxConvTensors] = {&g0, with_res ? &last_cb->gp : &g0, &g0};
  const void* sptr[kMaxConvTensors] = {cb.gps, with_res ? last_cb->gps : cb.gps, cb.gps};
  for (int sl = 0; sl < kMaxConvTensors; ++sl) set_conv_src(a, sl, *srcs[sl], x3 ? sptr[sl] : srcs[sl]->ptr);  // (the split layout keeps 4 bytes per channel: same strides)
  a.steps = dks;
  a.nsteps = (int)steps.size();
  a.w = wdev;
  a.bias = ts->zero_bias;
  a.out = out.ptr;
  if (x3) {
    a.w_lo = (const char*)wdev + wimg;
    cb.dx3 = true;
    // no bias, no ReLU, and the reader wants f32: the launch stores its raw sums (ConvArgs::raw, the epilogue of the
    // Winograd GEMMs) straight into the gradient tensor instead of (hi, lo) pairs that split_to_f32_kernel took apart again
    static const bool raw_out = env_on("BSMI_DGRAD_RAW");
    if (raw_out && out.Cpad % 4 == 0) {
      a.raw = 1;
    } else {
      rc = talloc(ts, &cb.dsplit, tensor_bytes(out), true);
      if (rc) return rc;
      a.out = cb.dsplit;
    }
  }
  a.Do = out.D; a.Ho = out.H; a.Wo = out.W; a.Co = out.Cpad;
  a.M = out.D * out.H * out.W;
  a.Npad = Npad;
  a.relu = 0;
  cb.need_dgrad = true;
  return BSMI_OK;
}

// backward data of the conv steps, in plan order; the first CONV step of the plan is the net's first conv
int make_conv_bwd(bsmi_unet* h, TrainState* ts) {
  Plan& plan = *ts->plan;
  const bool dgrad_x3 = h->train_split && env_on("BSMI_DGRAD_X3") && two_waves_per_simd();
  ts->convs.resize(plan.steps.size());
  bool first_conv = true;
  int rc;
  for (size_t i = 0; i < plan.steps.size(); ++i) {
    const PlanStep& st = plan.steps[i];
    if (st.type != PlanStep::CONV) continue;
    ConvBwd& cb = ts->convs[i];
    cb.st = &st;
    PassSite& p = *st.site;
    if ((rc = find_stage_params(ts, p.prefix, st.ci, &cb.par))) return rc;
    int crop[3];
    pass_crop(p, crop);
    for (int d = 0; d < 3; ++d) cb.P[d] = st.ci == p.nconv - 1 ? std::max(p.k[st.ci][d] - 1, crop[d] / 2) : p.k[st.ci][d] - 1;
    if (p.k[st.ci][2] > 3) BSMI_FAIL(BSMI_ERR_INVALID, "training: kernels wider than 3 along x are not supported");
    cb.gp = st.out;
    cb.gp.D += 2 * cb.P[0]; cb.gp.H += 2 * cb.P[1]; cb.gp.W += 2 * cb.P[2];
    const size_t bytes = tensor_bytes(cb.gp) + tensor_slack(cb.gp);
    if ((rc = talloc(ts, &cb.gp.ptr, bytes, true))) return rc;
    if (dgrad_x3 && (rc = talloc(ts, &cb.gps, bytes, true))) return rc;
    TDesc gy;
    if ((rc = grad_tensor(ts, st.out, &gy))) return rc;
    cb.need_dgrad = !(first_conv && st.ci == 0);
    first_conv = false;
  }
  // dgrad launches need the padded gradient of the pass's LAST stage (residual source): second sweep
  for (size_t i = 0; i < plan.steps.size(); ++i) {
    ConvBwd& cb = ts->convs[i];
    if (!cb.st || !cb.need_dgrad) continue;
    const ConvBwd* last_cb = nullptr;
    for (size_t j = i; j < plan.steps.size(); ++j)
      if (ts->convs[j].st && ts->convs[j].st->site == cb.st->site && ts->convs[j].st->ci == cb.st->site->nconv - 1) {
        last_cb = &ts->convs[j];
        break;
      }
    if (!last_cb) BSMI_FAIL(BSMI_ERR_STATE, "training plan: last stage of %s not found", cb.st->site->prefix.c_str());
    cb.need_dgrad = false;
    if ((rc = make_dgrad(ts, cb, last_cb))) return rc;
  }
  return BSMI_OK;
}

}  // namespace bsmi

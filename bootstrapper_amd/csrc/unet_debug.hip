// Debug entry points of the U-Net engine: what the last forward's plan looks like (bsmi_unet_debug_step_info) and what its
// steps left in their tensors (bsmi_unet_debug_activation).  The per-launch parity tests read both.
#include <cstring>

#include "unet_internal.h"

extern "C" {

int bsmi_debug_wino_pack_host(const float* w, int cout, int cin, int wz, uint16_t* out, uint64_t capacity, uint64_t* image_elems, uint64_t* batch_elems,
                              int* npad, int* ksteps) {
  if (!w || cout < 1 || cin < 1) BSMI_FAIL(BSMI_ERR_INVALID, "bad argument");
  std::vector<int> cin_of_v;
  for (int c = 0; c < round_up(cin, kChanPad); ++c) cin_of_v.push_back(c < cin ? c : -1);
  const int Npad = round_up(cout, tile_bn(choose_tile(cout)));
  std::vector<WinoUnit> units;
  wino_units((int)cin_of_v.size(), units, wz ? 1 : 3);
  if (image_elems || batch_elems || out) {
    std::vector<uint16_t> packed;
    size_t ie = 0, be = 0;
    wino_pack_weights(w, cout, cin, cin_of_v, Npad, units, packed, ie, be, 4, wz != 0);
    if (image_elems) *image_elems = ie;
    if (batch_elems) *batch_elems = be;
    if (out) {
      if (capacity < packed.size()) BSMI_FAIL(BSMI_ERR_INVALID, "buffer of %llu values too small", (unsigned long long)capacity);
      memcpy(out, packed.data(), packed.size() * sizeof(uint16_t));
    }
  }
  if (npad) *npad = Npad;
  if (ksteps) *ksteps = (int)(units.size() / kUnitsPerStep);
  return BSMI_OK;
}

int bsmi_unet_debug_activation(bsmi_unet* h, int step, int what, int64_t shape_out[4], float* host_out, uint64_t capacity) {
  if (!h || !shape_out) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Plan* plan = h->last_plan;
  if (!plan) BSMI_FAIL(BSMI_ERR_STATE, "no forward has run");
  if (step < 0 || step >= (int)plan->steps.size()) BSMI_FAIL(BSMI_ERR_INVALID, "step %d out of range (%zu steps)", step, plan->steps.size());
  const PlanStep& st = plan->steps[step];
  if (st.type == PlanStep::HEAD) BSMI_FAIL(BSMI_ERR_INVALID, "head steps write into the caller's buffers");
  if (plan->fused_first && step < 2)
    BSMI_FAIL(BSMI_ERR_STATE, "step %d is not materialised: the first ConvPass ran as one launch (first_pass), which writes step 2 only", step);
  if (st.type == PlanStep::UP && st.skip)
    BSMI_FAIL(BSMI_ERR_STATE, "step %d is not materialised: the upsampling is fused into the Winograd stages that read it", step);
  const TDesc& t = st.out;
  shape_out[0] = t.D; shape_out[1] = t.H; shape_out[2] = t.W; shape_out[3] = t.C;
  if (!host_out) return BSMI_OK;
  const size_t nvox = (size_t)t.D * t.H * t.W;
  if (capacity < nvox * t.C) BSMI_FAIL(BSMI_ERR_INVALID, "buffer of %llu floats too small", (unsigned long long)capacity);
  BSMI_HIP(hipSetDevice(h->device));
  BSMI_HIP(hipDeviceSynchronize());
  const int es = esize(plan->prec);
  const bool split = t.lo_off != 0;
  const size_t bytes = nvox * t.Cpad * es * (split ? 2 : 1);
  std::vector<uint8_t> raw(bytes);
  BSMI_HIP(hipMemcpy(raw.data(), t.ptr, raw.size(), hipMemcpyDeviceToHost));
  for (size_t v = 0; v < nvox; ++v)
    for (int c = 0; c < t.C; ++c) {
      float x;
      if (plan->prec == BSMI_PREC_F32) {
        x = ((const float*)raw.data())[v * t.Cpad + c];
      } else if (!split) {
        x = host_bf16_to_f32(((const uint16_t*)raw.data())[v * t.Cpad + c]);
      } else {  // (hi, lo) vectors of 8 interleaved
        const size_t i = 2 * v * t.Cpad + (size_t)((c >> 3) << 4) + (c & 7);
        const float hi = host_bf16_to_f32(((const uint16_t*)raw.data())[i]);
        const float lo = host_bf16_to_f32(((const uint16_t*)raw.data())[i + 8]);
        x = what == 1 ? hi : (what == 2 ? lo : hi + lo);
      }
      host_out[v * t.C + c] = x;
    }
  return BSMI_OK;
}

int bsmi_unet_debug_step_info(bsmi_unet* h, int step, bsmi_unet_step_info* info, int* n_steps) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  Plan* plan = h->last_plan;
  if (!plan) BSMI_FAIL(BSMI_ERR_STATE, "no forward has run");
  if (n_steps) *n_steps = (int)plan->steps.size();
  if (!info) return BSMI_OK;
  if (step < 0 || step >= (int)plan->steps.size()) BSMI_FAIL(BSMI_ERR_INVALID, "step %d out of range (%zu steps)", step, plan->steps.size());
  const PlanStep& st = plan->steps[step];
  memset(info, 0, sizeof *info);
  info->type = (int32_t)st.type;
  const bool in_first = plan->fused_first && step < 3;
  info->materialised = !((plan->fused_first && step < 2) || (st.type == PlanStep::UP && st.skip));
  const TDesc& t = st.type == PlanStep::HEAD ? st.in : st.out;
  info->shape[0] = t.D; info->shape[1] = t.H; info->shape[2] = t.W;
  info->shape[3] = st.type == PlanStep::HEAD ? h->heads[st.head].cout : t.C;
  const std::string* prefix = nullptr;
  if (st.type == PlanStep::HEAD) {
    info->head = st.head;
    prefix = &h->heads[st.head].prefix;
  } else if (st.type == PlanStep::POOL || st.type == PlanStep::UP) {
    for (int d = 0; d < 3; ++d) { info->factor[d] = st.f[d]; info->offset[d] = st.type == PlanStep::UP ? st.o[d] : 0; }
  } else if (st.type == PlanStep::CONV) {
    prefix = &st.site->prefix;
    info->conv_index = st.ci;
    const int sk_grid = h->sk_grid > 0 ? h->sk_grid : 0;
    if (in_first) {
      info->form = BSMI_FORM_FIRST_PASS;
    } else if (st.use_wino) {
      info->form = st.wino_in.m == 4 ? BSMI_FORM_WINO4 : BSMI_FORM_WINO2;
      info->bn = tile_bn(st.tile);
      info->ksteps = st.wino_gemm.nsteps;
      bool up = false;
      for (int q = 0; q < st.wino_in.nsrc; ++q) up = up || st.wino_in.upf[q] > 0;
      if (up || st.wino_out.low || st.wino_has_below) info->flags |= BSMI_STEP_FUSED_UP;
      if (st.wino_has_below) info->flags |= BSMI_STEP_BELOW_UP;
      if (st.wino_has_res_low) info->flags |= BSMI_STEP_RES_LOW;
      if (st.wino_in.wz) info->flags |= BSMI_STEP_WINO_Z;
      if (conv_igemm_split_k(st.wino_gemm, plan->prec, st.tile, sk_grid) ||
          (st.wino_has_res && conv_igemm_split_k(st.wino_res, plan->prec, st.tile, sk_grid)) ||
          (st.wino_has_res_low && conv_igemm_split_k(st.wino_res_low, plan->prec, st.tile, sk_grid)) ||
          (st.wino_has_below && conv_igemm_split_k(st.wino_below, plan->prec, st.below_tile, sk_grid)))
        info->flags |= BSMI_STEP_SPLIT_K;
    } else if (st.use_h16) {
      info->form = BSMI_FORM_HALO_RESIDENT;
      info->bn = st.h16.Npad;
      info->ksteps = st.h16.nsteps;
    } else if (st.use_box) {
      info->form = BSMI_FORM_BOX_HALO;
    } else if (st.use_rh) {
      info->form = BSMI_FORM_RASTER_HALO;
      info->bn = tile_bn(st.tile);
      info->ksteps = st.rh.nsteps;
      if (conv_rh_split_k(st.rh, st.tile, sk_grid)) info->flags |= BSMI_STEP_SPLIT_K;
    } else {
      info->form = BSMI_FORM_GATHER;
      info->bn = tile_bn(st.tile);
      info->ksteps = st.conv.nsteps;
      if (conv_igemm_split_k(st.conv, plan->prec, st.tile, sk_grid)) info->flags |= BSMI_STEP_SPLIT_K;
    }
  }
  if (prefix) snprintf(info->prefix, sizeof info->prefix, "%s", prefix->c_str());
  return BSMI_OK;
}

}  // extern "C"

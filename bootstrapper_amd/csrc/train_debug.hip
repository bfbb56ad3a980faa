// Training engine: the debug entry points, which the per-launch parity tests read (tests/test_backward_gpu.py): what the last
// pass launched per plan step, and the tensors a step leaves on the device (train_internal.h has the file map).
#include <cstring>

#include "train_internal.h"

extern "C" {

int bsmi_unet_train_debug_step_info(bsmi_unet* h, int step, bsmi_unet_train_step_info* info) {
  if (!h || !h->train || !info) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  if (step < 0 || step >= (int)h->train->rec.size()) BSMI_FAIL(BSMI_ERR_INVALID, "step %d out of range (%zu steps)", step, h->train->rec.size());
  *info = h->train->rec[step];
  return BSMI_OK;
}

int bsmi_unet_train_debug_tensor(bsmi_unet* h, int step, int what, int64_t shape_out[4], float* host_out, uint64_t capacity) {
  if (!h || !h->train || !shape_out) BSMI_FAIL(BSMI_ERR_STATE, "bsmi_unet_train_begin has not been called / null argument");
  TrainState* ts = h->train;
  Plan& plan = *ts->plan;
  if (step < 0 || step >= (int)plan.steps.size()) BSMI_FAIL(BSMI_ERR_INVALID, "step %d out of range (%zu steps)", step, plan.steps.size());
  const PlanStep& st = plan.steps[step];
  const ConvBwd* cb = st.type == PlanStep::CONV ? &ts->convs[step] : nullptr;
  BSMI_HIP(hipSetDevice(h->device));
  auto fetch = [&](const void* ptr, size_t floats, std::vector<float>& raw) -> int {
    raw.resize(floats);
    BSMI_HIP(hipDeviceSynchronize());  // every stream of the device, the weight gradients' own included
    BSMI_HIP(hipMemcpy(raw.data(), ptr, floats * sizeof(float), hipMemcpyDeviceToHost));
    return BSMI_OK;
  };
  auto find_grad = [&](const TDesc& act, TDesc* out) {
    auto it = ts->grad_of.find(act.ptr);
    if (it == ts->grad_of.end()) return false;
    *out = it->second;
    return true;
  };
  int rc;
  std::vector<float> raw;
  if (what == BSMI_TRAIN_DBG_HEAD_DP) {
    if (st.type != PlanStep::HEAD) BSMI_FAIL(BSMI_ERR_STATE, "step %d is no head", step);
    const int co = h->heads[st.head].cout;
    shape_out[0] = st.in.D; shape_out[1] = st.in.H; shape_out[2] = st.in.W; shape_out[3] = co;
    if (!host_out) return BSMI_OK;
    if (capacity < ts->out_vox * co) BSMI_FAIL(BSMI_ERR_INVALID, "buffer of %llu floats too small", (unsigned long long)capacity);
    if ((rc = fetch(ts->head_dp[st.head], ts->out_vox * co, raw))) return rc;
    for (size_t v = 0; v < ts->out_vox; ++v)
      for (int c = 0; c < co; ++c) host_out[v * co + c] = raw[(size_t)c * ts->out_vox + v];
    return BSMI_OK;
  }
  if (what == BSMI_TRAIN_DBG_PAD_COUNT) {
    if (!cb || !cb->st) BSMI_FAIL(BSMI_ERR_STATE, "step %d is no conv step", step);
    shape_out[0] = shape_out[1] = shape_out[2] = 1; shape_out[3] = 4;
    if (!host_out) return BSMI_OK;
    if (capacity < 4) BSMI_FAIL(BSMI_ERR_INVALID, "buffer of %llu floats too small", (unsigned long long)capacity);
    auto pad_channels = [&](const TDesc& t, const std::vector<float>& a) {
      size_t cnt = 0;
      const size_t nv = (size_t)t.D * t.H * t.W;
      for (size_t v = 0; v < nv; ++v)
        for (int c = t.C; c < t.Cpad; ++c) cnt += a[v * t.Cpad + c] != 0.f;
      return cnt;
    };
    const TDesc& g = cb->gp;
    if ((rc = fetch(g.ptr, (size_t)g.D * g.H * g.W * g.Cpad, raw))) return rc;
    host_out[0] = (float)pad_channels(g, raw);
    size_t border = 0;
    for (int z = 0; z < g.D; ++z)
      for (int y = 0; y < g.H; ++y)
        for (int x = 0; x < g.W; ++x) {
          const bool inside = z >= cb->P[0] && z < g.D - cb->P[0] && y >= cb->P[1] && y < g.H - cb->P[1] && x >= cb->P[2] && x < g.W - cb->P[2];
          if (inside) continue;
          const float* r = raw.data() + (((size_t)z * g.H + y) * g.W + x) * g.Cpad;
          for (int c = 0; c < g.Cpad; ++c) border += r[c] != 0.f;
        }
    host_out[1] = (float)border;
    TDesc gy;
    host_out[2] = 0.f;
    if (find_grad(st.out, &gy)) {
      if ((rc = fetch(gy.ptr, (size_t)gy.D * gy.H * gy.W * gy.Cpad, raw))) return rc;
      host_out[2] = (float)pad_channels(gy, raw);
    }
    host_out[3] = 0.f;
    if (cb->dcat.ptr) {
      if ((rc = fetch(cb->dcat.ptr, (size_t)cb->dcat.D * cb->dcat.H * cb->dcat.W * cb->dcat.Cpad, raw))) return rc;
      host_out[3] = (float)pad_channels(cb->dcat, raw);
    }
    return BSMI_OK;
  }
  TDesc t;
  bool split = false;
  switch (what) {
    case BSMI_TRAIN_DBG_DOUT:
      if (st.type == PlanStep::HEAD || !find_grad(st.out, &t)) BSMI_FAIL(BSMI_ERR_STATE, "step %d has no output gradient tensor", step);
      break;
    case BSMI_TRAIN_DBG_GMASK:
      if (!cb || !cb->st) BSMI_FAIL(BSMI_ERR_STATE, "step %d is no conv step", step);
      t = cb->gp;
      break;
    case BSMI_TRAIN_DBG_GSPLIT: case BSMI_TRAIN_DBG_GSPLIT_HI: case BSMI_TRAIN_DBG_GSPLIT_LO:
      if (!cb || !cb->st || !cb->gps) BSMI_FAIL(BSMI_ERR_STATE, "step %d has no split copy of its masked gradient", step);
      t = cb->gp;
      t.ptr = cb->gps;
      split = true;
      break;
    case BSMI_TRAIN_DBG_DCAT:
      if (!cb || !cb->st || !cb->scatter || !cb->dcat.ptr) BSMI_FAIL(BSMI_ERR_STATE, "step %d has no concat-input gradient", step);
      t = cb->dcat;
      break;
    default: BSMI_FAIL(BSMI_ERR_INVALID, "unknown tensor %d", what);
  }
  shape_out[0] = t.D; shape_out[1] = t.H; shape_out[2] = t.W; shape_out[3] = t.C;
  if (!host_out) return BSMI_OK;
  const size_t nvox = (size_t)t.D * t.H * t.W;
  if (capacity < nvox * t.C) BSMI_FAIL(BSMI_ERR_INVALID, "buffer of %llu floats too small", (unsigned long long)capacity);
  if ((rc = fetch(t.ptr, nvox * t.Cpad, raw))) return rc;  // (the split layout keeps 4 bytes per channel)
  const uint16_t* r16 = (const uint16_t*)raw.data();
  auto bf16_value = [](uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
  };
  for (size_t v = 0; v < nvox; ++v)
    for (int c = 0; c < t.C; ++c) {
      float x;
      if (!split) {
        x = raw[v * t.Cpad + c];
      } else {  // (hi, lo) vectors of 8 interleaved (conv_dev.h act_index)
        const size_t i = 2 * v * t.Cpad + (size_t)((c >> 3) << 4) + (c & 7);
        const float hi = bf16_value(r16[i]), lo = bf16_value(r16[i + 8]);
        x = what == BSMI_TRAIN_DBG_GSPLIT_HI ? hi : (what == BSMI_TRAIN_DBG_GSPLIT_LO ? lo : hi + lo);
      }
      host_out[v * t.C + c] = x;
    }
  return BSMI_OK;
}

}  // extern "C"

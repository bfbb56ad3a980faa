// Host side of the U-Net engine: network description, the handle's life cycle and the
// C-ABI entry points declared in include/bsmi.h that are neither the forward pass (unet_forward.hip) nor debug reads
// (unet_debug.hip).  unet_internal.h lists the engine's translation units.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include <chrono>
#include <thread>

#include "unet_internal.h"
#include "unet_ops.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

static void expect_weight(bsmi_unet* h, const std::string& key, std::vector<int64_t> shape) {
  HostWeight hw;
  hw.shape = std::move(shape);
  h->weights[key] = std::move(hw);
}

static void register_pass(bsmi_unet* h, const PassSite& p) {
  int cin_total = p.cin[0] + (p.nslots > 1 ? p.cin[1] : 0);
  int cin = cin_total;
  for (int i = 0; i < p.nconv; ++i) {
    const std::string base = p.prefix + ".conv_pass." + std::to_string(2 * i);
    expect_weight(h, base + ".weight", {p.cout, cin, p.k[i][0], p.k[i][1], p.k[i][2]});
    expect_weight(h, base + ".bias", {p.cout});
    cin = p.cout;
  }
  expect_weight(h, p.prefix + ".residual.0.weight", {p.cout, cin_total, 1, 1, 1});
  expect_weight(h, p.prefix + ".residual.0.bias", {p.cout});
}

}  // namespace bsmi

extern "C" {

const char* bsmi_last_error(void) { return g_err.c_str(); }
int bsmi_version(void) { return 1; }

int bsmi_unet_create(const bsmi_unet_config* cfg, int device, bsmi_unet** out) {
  if (!cfg || !out) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  if (cfg->num_levels < 1 || cfg->num_levels > BSMI_MAX_LEVELS) BSMI_FAIL(BSMI_ERR_INVALID, "num_levels %d out of range", cfg->num_levels);
  if (cfg->num_heads < 1 || cfg->num_heads > BSMI_MAX_HEADS) BSMI_FAIL(BSMI_ERR_INVALID, "num_heads %d out of range", cfg->num_heads);
  if (cfg->in_channels < 1 || cfg->num_fmaps < 1 || cfg->fmap_inc_factor < 1 || cfg->num_fmaps_out < 0) BSMI_FAIL(BSMI_ERR_INVALID, "bad channel configuration");
  // no HIP call here: shape / flop arithmetic must work on a host without a GPU
  std::unique_ptr<bsmi_unet> h(new bsmi_unet);
  h->cfg = *cfg;
  h->device = device;
  h->nl = cfg->num_levels;
  auto fm = [&](int level) {
    int64_t c = cfg->num_fmaps;
    for (int i = 0; i < level; ++i) c *= cfg->fmap_inc_factor;
    return (int)c;
  };
  auto fill_k = [&](PassSite& p, int n, const int32_t (*k)[3]) -> int {
    if (n < 1 || n > BSMI_MAX_CONVS) BSMI_FAIL(BSMI_ERR_INVALID, "%s: %d convolutions per pass unsupported", p.prefix.c_str(), n);
    p.nconv = n;
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < 3; ++d) {
        if (k[i][d] < 1 || k[i][d] > 7) BSMI_FAIL(BSMI_ERR_INVALID, "%s: kernel size %d unsupported", p.prefix.c_str(), k[i][d]);
        p.k[i][d] = k[i][d];
      }
    return BSMI_OK;
  };
  for (int l = 0; l < h->nl; ++l) {
    PassSite p;
    p.prefix = "unet.l_conv." + std::to_string(l);
    p.nslots = 1;
    p.cin[0] = l == 0 ? cfg->in_channels : fm(l - 1);
    p.cout = fm(l);
    int rc = fill_k(p, cfg->n_convs_down[l], cfg->kernel_size_down[l]);
    if (rc) return rc;
    h->l_conv.push_back(p);
  }
  for (int l = 0; l < h->nl - 1; ++l) {
    PassSite p;
    p.prefix = "unet.r_conv.0." + std::to_string(l);
    p.nslots = 2;
    p.cin[0] = fm(l);      // skip connection first (torch.cat([f_cropped, g_cropped]), unet.py:223)
    p.cin[1] = fm(l + 1);
    p.cout = (l == 0 && cfg->num_fmaps_out > 0) ? cfg->num_fmaps_out : fm(l);  // unet.py:426-427
    int rc = fill_k(p, cfg->n_convs_up[l], cfg->kernel_size_up[l]);
    if (rc) return rc;
    h->r_conv.push_back(p);
  }
  // crop factors (unet.py:353-362): running product of the downsample factors from the bottom
  {
    int prod[3] = {1, 1, 1};
    for (int l = h->nl - 2; l >= 0; --l) {
      for (int d = 0; d < 3; ++d) {
        if (cfg->downsample_factors[l][d] < 1) BSMI_FAIL(BSMI_ERR_INVALID, "bad downsample factor");
        prod[d] *= cfg->downsample_factors[l][d];
        h->crop_factor[l][d] = prod[d];
      }
    }
  }
  for (auto& p : h->l_conv) register_pass(h.get(), p);
  for (auto& p : h->r_conv) register_pass(h.get(), p);
  for (int i = 0; i < cfg->num_heads; ++i) {
    HeadSite hs;
    hs.prefix = std::string(cfg->head_name[i], strnlen(cfg->head_name[i], BSMI_NAME_LEN));
    hs.cin = (cfg->num_fmaps_out > 0 && h->nl > 1) ? cfg->num_fmaps_out : cfg->num_fmaps;
    hs.cout = cfg->head_dims[i];
    if (hs.cout < 1 || hs.cout > 64) BSMI_FAIL(BSMI_ERR_INVALID, "head %s: dims %d unsupported", hs.prefix.c_str(), hs.cout);
    expect_weight(h.get(), hs.prefix + ".conv_pass.0.weight", {hs.cout, hs.cin, 1, 1, 1});
    expect_weight(h.get(), hs.prefix + ".conv_pass.0.bias", {hs.cout});
    expect_weight(h.get(), hs.prefix + ".residual.0.weight", {hs.cout, hs.cin, 1, 1, 1});
    expect_weight(h.get(), hs.prefix + ".residual.0.bias", {hs.cout});
    h->heads.push_back(hs);
  }
  *out = h.release();
  return BSMI_OK;
}

int bsmi_stream_create_cu_mask(int device, const uint32_t* cu_mask, int n_words, void** stream_out) {
  if (!stream_out || (cu_mask && n_words < 1)) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  BSMI_HIP(hipSetDevice(device));
  hipStream_t s = nullptr;
  if (!cu_mask) BSMI_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));  // an ordinary stream the caller may destroy again
  else BSMI_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, cu_mask));
  *stream_out = (void*)s;
  return BSMI_OK;
}

int bsmi_stream_destroy(int device, void* stream) {
  if (!stream) return BSMI_OK;
  BSMI_HIP(hipSetDevice(device));
  BSMI_HIP(hipStreamDestroy((hipStream_t)stream));
  return BSMI_OK;
}

int bsmi_unet_set_persistent_grid(bsmi_unet* h, int n_cus) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  if (n_cus < -1) BSMI_FAIL(BSMI_ERR_INVALID, "n_cus must be >= -1");
  BSMI_HIP(hipSetDevice(h->device));
  if (h->sk_ws) {
    BSMI_HIP(hipDeviceSynchronize());
    BSMI_HIP(hipFree(h->sk_ws));
    h->sk_ws = nullptr;
  }
  h->sk_grid = 0;
  h->sk_request = n_cus < 0 ? -1 : n_cus / 8 * 8;
  return BSMI_OK;
}

int bsmi_unet_destroy(bsmi_unet* h) {
  if (!h) return BSMI_OK;
  (void)hipSetDevice(h->device);
  for (auto& kv : h->plans) free_plan(kv.second.get());
  for (auto* sites : {&h->l_conv, &h->r_conv})
    for (PassSite& p : *sites)
      for (int c = 0; c < BSMI_MAX_CONVS; ++c) {
        for (int pr = 0; pr < BSMI_NUM_PREC; ++pr) release(p.packed[pr][c]);
        release(p.h16[c]);
        release(p.wino[c]);
      }
  free_train_state(h);
  free_first_pass(h->first_pass);
  free_first_pass(h->first_pass_x3);
  if (h->sk_ws) (void)hipFree(h->sk_ws);
  for (auto& hd : h->heads) {
    if (hd.hw) (void)hipFree(hd.hw);
    if (hd.hb) (void)hipFree(hd.hb);
  }
  delete h;
  return BSMI_OK;
}

int bsmi_unet_load_weight(bsmi_unet* h, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!h || !key || !data || !shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  auto it = h->weights.find(key);
  if (it == h->weights.end()) BSMI_FAIL(BSMI_ERR_MISSING, "Unexpected key(s) in state_dict: \"%s\"", key);
  HostWeight& w = it->second;
  bool ok = (size_t)ndim == w.shape.size();
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == w.shape[i];
  if (!ok) {
    std::string got, want;
    for (int i = 0; i < ndim; ++i) got += std::to_string(shape[i]) + (i + 1 < ndim ? ", " : "");
    for (size_t i = 0; i < w.shape.size(); ++i) want += std::to_string(w.shape[i]) + (i + 1 < w.shape.size() ? ", " : "");
    BSMI_FAIL(BSMI_ERR_INVALID, "size mismatch for %s: copying a param with shape (%s), the shape in current model is (%s)",
              key, got.c_str(), want.c_str());
  }
  size_t n = 1;
  for (auto s : w.shape) n *= (size_t)s;
  w.data.assign(data, data + n);
  w.loaded = true;
  // weights changed: packed copies are stale
  for (int pr = 0; pr < BSMI_NUM_PREC; ++pr) h->finalized[pr] = false;
  return BSMI_OK;
}

int bsmi_unet_finalize(bsmi_unet* h, int precision) {
  if (!h) BSMI_FAIL(BSMI_ERR_INVALID, "null handle");
  if (precision < 0 || precision >= BSMI_NUM_PREC) BSMI_FAIL(BSMI_ERR_INVALID, "unknown precision %d", precision);
  std::string missing;
  for (auto& kv : h->weights)
    if (!kv.second.loaded) missing += (missing.empty() ? "\"" : ", \"") + kv.first + "\"";
  if (!missing.empty()) BSMI_FAIL(BSMI_ERR_MISSING, "Missing key(s) in state_dict: %s", missing.c_str());
  // launch_head's limit, refused here: a wider net would otherwise run its whole trunk and fail at the last launch of a forward
  for (auto& hd : h->heads)
    if (round_up(hd.cin, kChanPad) > 64)
      BSMI_FAIL(BSMI_ERR_INVALID, "head kernel supports at most 64 input channels (%s reads %d)", hd.prefix.c_str(), hd.cin);
  BSMI_HIP(hipSetDevice(h->device));
  auto repack = [&](PassSite& p) -> int {
    for (int c = 0; c < p.nconv; ++c) {
      release(p.packed[precision][c]);
      int rc = pack_conv(h, p, c, precision);
      if (rc) return rc;
      if (precision == BSMI_PREC_BF16X3 && (rc = pack_wino(h, p, c))) return rc;
      if (precision == BSMI_PREC_BF16X3 && (rc = pack_h16(h, p, c))) return rc;
    }
    return BSMI_OK;
  };
  {
    // the ConvPasses side by side (each packs its stages on host threads of its own and uploads its images): the 1500-channel
    // pass alone is two thirds of the work, the others hide behind it
    std::vector<PassSite*> sites;
    for (auto& p : h->l_conv) sites.push_back(&p);
    for (auto& p : h->r_conv) sites.push_back(&p);
    std::vector<int> rcs(sites.size(), BSMI_OK);
    std::vector<std::string> msgs(sites.size());
    const bool timing = getenv("BSMI_PLAN_DEBUG") != nullptr;
    std::vector<std::thread> th;
    for (size_t i = 0; i < sites.size(); ++i)
      th.emplace_back([&, i] {
        (void)hipSetDevice(h->device);
        const auto t0 = std::chrono::steady_clock::now();
        rcs[i] = repack(*sites[i]);
        if (rcs[i]) msgs[i] = bsmi_last_error();
        if (timing) fprintf(stderr, "[bsmi finalize] %s: %.3f s\n", sites[i]->prefix.c_str(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
      });
    for (auto& t : th) t.join();
    for (size_t i = 0; i < sites.size(); ++i)
      if (rcs[i]) { bsmi::set_error("%s", msgs[i].c_str()); return rcs[i]; }
  }
  for (auto& hd : h->heads) {
    std::vector<float> hw((size_t)hd.cout * 2 * hd.cin), hb((size_t)hd.cout * 2);
    const HostWeight& w1 = h->weights[hd.prefix + ".conv_pass.0.weight"];
    const HostWeight& b1 = h->weights[hd.prefix + ".conv_pass.0.bias"];
    const HostWeight& w2 = h->weights[hd.prefix + ".residual.0.weight"];
    const HostWeight& b2 = h->weights[hd.prefix + ".residual.0.bias"];
    for (int o = 0; o < hd.cout; ++o) {
      for (int c = 0; c < hd.cin; ++c) {
        hw[((size_t)o * 2 + 0) * hd.cin + c] = w1.data[(size_t)o * hd.cin + c];
        hw[((size_t)o * 2 + 1) * hd.cin + c] = w2.data[(size_t)o * hd.cin + c];
      }
      hb[o * 2] = b1.data[o];
      hb[o * 2 + 1] = b2.data[o];
    }
    if (!hd.hw) BSMI_HIP(hipMalloc((void**)&hd.hw, hw.size() * sizeof(float)));
    if (!hd.hb) BSMI_HIP(hipMalloc((void**)&hd.hb, hb.size() * sizeof(float)));
    BSMI_HIP(hipMemcpy(hd.hw, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice));
    BSMI_HIP(hipMemcpy(hd.hb, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if ((precision == BSMI_PREC_BF16 || precision == BSMI_PREC_BF16X3) && first_pass_eligible(h)) {
    const std::string pre = h->l_conv[0].prefix;
    const bool split = precision == BSMI_PREC_BF16X3;
    int rc = pack_first_pass(split ? h->first_pass_x3 : h->first_pass, h->l_conv[0].cout, h->weights[pre + ".conv_pass.0.weight"].data.data(),
                             h->weights[pre + ".conv_pass.0.bias"].data.data(), h->weights[pre + ".conv_pass.2.weight"].data.data(),
                             h->weights[pre + ".conv_pass.2.bias"].data.data(), h->weights[pre + ".residual.0.weight"].data.data(),
                             h->weights[pre + ".residual.0.bias"].data.data(), split);
    if (rc) return rc;
  }
  // plans hold pointers to packed weights: drop those of this precision
  h->last_plan = nullptr;
  for (auto it = h->plans.begin(); it != h->plans.end();) {
    if (it->first[0] == precision) { free_plan(it->second.get()); it = h->plans.erase(it); }
    else ++it;
  }
  h->finalized[precision] = true;
  return BSMI_OK;
}

int bsmi_unet_output_shape(bsmi_unet* h, const int64_t in_shape[3], int64_t out_shape[3]) {
  if (!h || !in_shape || !out_shape) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Plan plan;
  int rc = dry_plan(h, in_shape, plan);
  if (rc) return rc;
  for (int d = 0; d < 3; ++d) out_shape[d] = plan.out_shape[d];
  return BSMI_OK;
}

int bsmi_unet_flops(bsmi_unet* h, const int64_t in_shape[3], double* flops) {
  if (!h || !in_shape || !flops) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  Plan plan;
  int rc = dry_plan(h, in_shape, plan);
  if (rc) return rc;
  *flops = plan.flops;
  return BSMI_OK;
}

int bsmi_extract_block_reflect_u8(const uint8_t* vol_dev, const int64_t vol_shape[3], const int64_t offset[3],
                                  const int64_t block_shape[3], uint8_t* block_dev, void* stream) {
  if (!vol_dev || !vol_shape || !offset || !block_shape || !block_dev) BSMI_FAIL(BSMI_ERR_INVALID, "null argument");
  for (int d = 0; d < 3; ++d)
    if (vol_shape[d] <= 0 || block_shape[d] <= 0 || vol_shape[d] > (1 << 20) || block_shape[d] > (1 << 20))
      BSMI_FAIL(BSMI_ERR_INVALID, "bad shape");
  return launch_extract_block_reflect(vol_dev, vol_shape, offset, block_shape, block_dev, (hipStream_t)stream);
}

}  // extern "C"

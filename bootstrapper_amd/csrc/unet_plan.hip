// The planner of the U-Net engine.  It restates the control flow of the reference UNet.rec_forward
// (models/3d_affs/unet.py:440-469) once per input shape and lowers it to a flat list of
// launches: every ConvPass stage (unet.py:7-76) becomes ONE implicit-GEMM launch whose
// K-steps cover the kernel taps of all concatenated inputs plus, for the last stage, the
// cropped 1x1x1 residual branch; max-pool and trilinear-upsample+crop are separate
// memory-bound launches; the crop of the skip connection (unet.py:203-213) is pure index
// arithmetic folded into the K-step offsets.  The Winograd form of a stage is in unet_plan_wino.hip; which form a stage
// takes is decided by unet_rules.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "unet_plan.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

int upload_ksteps(Plan* plan, const std::vector<KStep>& ks, ConvArgs& a) {
  KStep* dks = nullptr;
  BSMI_HIP(hipMalloc((void**)&dks, ks.size() * sizeof(KStep)));
  plan->allocs.push_back(dks);
  BSMI_HIP(hipMemcpy(dks, ks.data(), ks.size() * sizeof(KStep), hipMemcpyHostToDevice));
  a.steps = dks;
  a.nsteps = (int)ks.size();
  return BSMI_OK;
}

void set_strides(ConvArgs& a, const void* base, int H, int W, int C, int bytes_per_channel) {
  for (int sl = 0; sl < kMaxConvTensors; ++sl) {
    a.t[sl].base = (uint64_t)(uintptr_t)base;
    a.t[sl].sz = (int32_t)((int64_t)H * W * C * bytes_per_channel);
    a.t[sl].sy = (int32_t)((int64_t)W * C * bytes_per_channel);
    a.t[sl].sx = (int32_t)((int64_t)C * bytes_per_channel);
  }
}

int Planner::alloc(TDesc& t) {
  t.Cpad = round_up(t.C, kChanPad);
  const size_t plane = (size_t)t.D * t.H * t.W * t.Cpad * esize(prec);
  const bool split = prec == BSMI_PREC_BF16X3;
  // split mode: each 16-byte vector of 8 hi values is followed by the 16 bytes of their lo values (conv_dev.h act_index)
  t.lo_off = split ? 16 : 0;
  const size_t bytes = split ? 2 * plane : plane;
  plan->bytes += bytes;
  if (bytes >= ((size_t)1 << 31))
    BSMI_FAIL(BSMI_ERR_INVALID, "activation tensor of %zu bytes exceeds the 31-bit byte offsets of the conv kernel", bytes);
  if (dry) return BSMI_OK;
  // slack: the raster-halo kernel stages whole rows of the input raster, and the rows it drops
  // (xx >= Wo, yy >= Ho) may lie a few lines past the end of a cropped source tensor
  const size_t slack = (size_t)8 * t.W * t.Cpad * esize(prec) * (split ? 2 : 1) + 4096;
  BSMI_HIP(hipMalloc(&t.ptr, bytes + slack));
  BSMI_HIP(hipMemsetAsync((char*)t.ptr + bytes, 0, slack, nullptr));
  plan->allocs.push_back(t.ptr);
  return BSMI_OK;
}

// Raster-halo launch of one ConvPass stage (conv_rh.hip) when the tile's halo buffer holds
// 256 + (ky-1)*Win + (kx-1) rows; otherwise st.use_rh stays false (gather kernel, conv_igemm.hip).
int Planner::plan_rh(const PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st) {
  st.use_rh = false;
  const bool enabled = rh_enabled(prec, st.tile, pc.entries.size() / kUnitsPerStep);
  const int* k = p.k[ci];
  const int Hin = o.H + k[1] - 1, Win = o.W + k[2] - 1;
  if (!enabled || !two_waves_per_simd() || !rh_supported(st.tile, Win, k[1], k[2])) return BSMI_OK;
  const int64_t es = esize(prec);  // bytes per channel of a row
  const int SUB = sube(prec);
  const size_t nsteps = pc.entries.size() / kUnitsPerStep;
  std::vector<RhStep> steps(nsteps);
  std::vector<RhPhase> phases;
  std::vector<int> first_step;  // per phase
  // phase key of the previous K-step
  int pslot = -1, pc32 = -1, pz = -1, pkind = -1;
  for (size_t s = 0; s < nsteps; ++s) {
    const PackEntry& e0 = pc.entries[kUnitsPerStep * s];
    const PackEntry& e1 = pc.entries[kUnitsPerStep * s + 1];
    if (e0.dummy) {  // the all-zero K-step that makes the count even: any resident halo row will do
      if (phases.empty() || !e1.dummy) BSMI_FAIL(BSMI_ERR_STATE, "raster-halo plan: K-step %zu starts with a padding unit", s);
      steps[s] = RhStep{0, (int32_t)(((phases.size() - 1) & 1) | ((phases.size() - 1) << 8)), 0, -1};
      continue;
    }
    const TDesc& t = slots[e0.slot];
    const int c32 = e0.c0 / (kUnitsPerStep * SUB) * (kUnitsPerStep * SUB);
    const int kind = e0.wsrc;
    if (!e1.dummy) {
      const bool same_tap = e1.dz == e0.dz && e1.dy == e0.dy && e1.dx == e0.dx && e1.c0 == e0.c0 + SUB && e1.slot == e0.slot;
      const bool x_pair = t.Cpad == SUB && e1.slot == e0.slot && e1.dz == e0.dz && e1.dy == e0.dy && e1.dx == e0.dx + 1 &&
                          e1.c0 == e0.c0 && kind == 0 && e1.wsrc == 0;
      if (!same_tap && !x_pair) return BSMI_OK;  // unit order the halo rows cannot serve: gather kernel
    }
    if (e0.slot != pslot || c32 != pc32 || e0.dz != pz || kind != pkind) {
      RhPhase ph;
      ph.tensor = e0.slot;
      const int oz = so[e0.slot][0] + e0.dz;
      const int oy = so[e0.slot][1] + (kind ? e0.dy : 0);
      const int ox = so[e0.slot][2] + (kind ? e0.dx : 0);
      ph.delta = (int32_t)(((((int64_t)oz * t.H + oy) * t.W + ox) * t.Cpad + c32) * es);
      ph.buf = (int32_t)(phases.size() & 1);
      ph.issue_step = -1;
      phases.push_back(ph);
      first_step.push_back((int)s);
      pslot = e0.slot; pc32 = c32; pz = e0.dz; pkind = kind;
    }
    RhStep& r = steps[s];
    r.rowoff = kind ? 0 : e0.dy * Win + e0.dx;
    r.buf_phase = (int32_t)(((phases.size() - 1) & 1) | ((phases.size() - 1) << 8));
    r.wait = 0;
    r.issue = -1;
  }
  const size_t nlisted = steps.size();
  const int np = (int)phases.size();
  // the halo of phase p >= 2 is staged with the weights of K-step issue_step + 4, as soon as
  // phase p-2 (same buffer) has been read; phases 0 and 1 in the prologue
  for (int q = 2; q < np; ++q) {
    const int is = first_step[q - 1] - 1;
    phases[q].issue_step = is;
    if (steps[is].issue >= 0) BSMI_FAIL(BSMI_ERR_STATE, "raster-halo plan: two halos on one staging slot");
    steps[is].issue = q;
  }
  // in-order queue of one wave: H0 [H1] W0 W1 W2 W3 {[H(issue[h])] W(h+4)}...
  std::vector<int> posW(nlisted + 8, 0), posH(np, 0);
  std::vector<char> isH;  // per queue position
  auto push = [&](bool halo) { isH.push_back(halo ? 1 : 0); return (int)isH.size() - 1; };
  posH[0] = push(true);
  if (np > 1) posH[1] = push(true);
  for (int w = 0; w < 4; ++w) posW[w] = push(false);
  for (size_t hh = 0; hh < nlisted; ++hh) {
    if (steps[hh].issue >= 0) posH[steps[hh].issue] = push(true);
    posW[hh + 4] = push(false);
  }
  for (size_t hh = 0; hh < nlisted; ++hh) {
    const int upto = posW[hh + 3];
    int need = posW[hh + 1];
    if (hh + 1 < nlisted) need = std::max(need, posH[steps[hh + 1].buf_phase >> 8]);
    if (need > upto) BSMI_FAIL(BSMI_ERR_STATE, "raster-halo plan: halo of K-step %zu staged too late", hh + 1);
    int aw = 0, bh = 0;
    for (int q = need + 1; q <= upto; ++q) (isH[q] ? bh : aw)++;
    if (aw > 2 || bh > 2) BSMI_FAIL(BSMI_ERR_STATE, "raster-halo plan: wait code out of range");
    steps[hh].wait = aw * 3 + bh;
  }
  RhArgs& a = st.rh;
  memset(&a, 0, sizeof a);
  for (int sl = 0; sl < kMaxConvTensors; ++sl) a.t[sl] = st.conv.t[sl];
  RhStep* dsteps = nullptr;
  RhPhase* dphases = nullptr;
  BSMI_HIP(hipMalloc((void**)&dsteps, steps.size() * sizeof(RhStep)));
  plan->allocs.push_back(dsteps);
  BSMI_HIP(hipMalloc((void**)&dphases, phases.size() * sizeof(RhPhase)));
  plan->allocs.push_back(dphases);
  BSMI_HIP(hipMemcpy(dsteps, steps.data(), steps.size() * sizeof(RhStep), hipMemcpyHostToDevice));
  BSMI_HIP(hipMemcpy(dphases, phases.data(), phases.size() * sizeof(RhPhase), hipMemcpyHostToDevice));
  a.steps = dsteps;
  a.phases = dphases;
  a.nsteps = (int)nlisted;
  a.nphases = np;
  a.w = pc.w;
  a.bias = pc.bias;
  a.out = o.ptr;
  a.Do = o.D; a.Ho = o.H; a.Wo = o.W; a.Co = o.Cpad;
  a.Hin = Hin; a.Win = Win;
  a.Q = o.D * Hin * Win;
  a.Npad = pc.Npad;
  a.relu = 1;
  st.use_rh = true;
  return BSMI_OK;
}

// Halo-resident launch of a stage with at most 64 output channels (conv_h16.hip), split-bf16 mode.
int Planner::plan_h16(PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st) {
  st.use_h16 = false;
  const PackedH16& ph = p.h16[ci];
  const int* k = p.k[ci];
  const int Hin = o.H + k[1] - 1, Win = o.W + k[2] - 1;
  if (prec != BSMI_PREC_BF16X3 || !ph.ready || h16_mode() == 0 || pc.bias == nullptr) return BSMI_OK;
  if (h16_only_npad() && h16_only_npad() != ph.Npad) return BSMI_OK;
  int max_r = 0;
  const int rows = h16_halo_rows(Win, k[1], k[2], ph.Npad, &max_r);
  if (!rows || Hin > 2047 || Win > 2047 || o.D > 1023) return BSMI_OK;
  const int64_t Q = (int64_t)o.D * Hin * Win;
  if (Q >= ((int64_t)1 << 31)) return BSMI_OK;
  // a launch that cannot fill the chip (two workgroups of 512 rows per CU) stays with the gather kernel's 256-row tiles
  if (h16_mode() == 1 && Q < (int64_t)2 * 256 * kH16TileRows) return BSMI_OK;
  // A residual branch costs this form one phase -- a halo load -- per 16 channels for half a K-step's worth of multiplies.
  // The second stage of unet.r_conv.0.1 (60 -> 60 channels, residual from 360): 23 such phases beside 12 of nine taps,
  // 0.60 ms against 0.56 for the gather kernel.
  if (h16_mode() == 1 && ph.Npad == 64) {
    int main_steps = 0, res_steps = 0;
    for (const H16PhaseHost& hp : ph.phases) (hp.kind ? res_steps : main_steps) += hp.nsteps;
    if (3 * res_steps > main_steps) return BSMI_OK;
  }
  const int64_t es = 4;  // bytes per channel of a row: (hi, lo) interleaved
  std::vector<H16Phase> phases(ph.phases.size());
  std::vector<H16Step> steps(ph.entries.size() / kUnitsPerStep);
  for (size_t q = 0; q < ph.phases.size(); ++q) {
    const H16PhaseHost& hp = ph.phases[q];
    const TDesc& t = slots[hp.slot];
    const PackEntry& e0 = ph.entries[(size_t)kUnitsPerStep * hp.first_step];
    // kind 0: the taps' (dy, dx) are row offsets into the halo; kind 1 (the residual's crop centre): folded into the origin
    const int oz = so[hp.slot][0] + hp.dz;
    const int oy = so[hp.slot][1] + (hp.kind ? e0.dy : 0);
    const int ox = so[hp.slot][2] + (hp.kind ? e0.dx : 0);
    const int64_t delta = ((((int64_t)oz * t.H + oy) * t.W + ox) * t.Cpad + hp.c0) * es;
    if (delta >= ((int64_t)1 << 31)) return BSMI_OK;
    phases[q] = H16Phase{hp.slot, (int32_t)delta, hp.kind ? kH16TileRows : kH16TileRows + (k[1] - 1) * Win + (k[2] - 1), hp.nsteps};
    for (int s = hp.first_step; s < hp.first_step + hp.nsteps; ++s) {
      const PackEntry& ea = ph.entries[(size_t)kUnitsPerStep * s];
      const PackEntry& eb = ph.entries[(size_t)kUnitsPerStep * s + 1];
      const int offa = hp.kind ? 0 : ea.dy * Win + ea.dx;
      const int offb = (hp.kind || eb.dummy) ? offa : eb.dy * Win + eb.dx;
      steps[s] = H16Step{offa, offb, 0, 0};
    }
  }
  H16Args& a = st.h16;
  memset(&a, 0, sizeof a);
  for (int sl = 0; sl < kMaxConvTensors; ++sl) a.t[sl] = st.conv.t[sl];
  H16Phase* dphases = nullptr;
  H16Step* dsteps = nullptr;
  BSMI_HIP(hipMalloc((void**)&dphases, phases.size() * sizeof(H16Phase)));
  plan->allocs.push_back(dphases);
  BSMI_HIP(hipMalloc((void**)&dsteps, steps.size() * sizeof(H16Step)));
  plan->allocs.push_back(dsteps);
  BSMI_HIP(hipMemcpy(dphases, phases.data(), phases.size() * sizeof(H16Phase), hipMemcpyHostToDevice));
  BSMI_HIP(hipMemcpy(dsteps, steps.data(), steps.size() * sizeof(H16Step), hipMemcpyHostToDevice));
  a.phases = dphases;
  a.steps = dsteps;
  a.nphases = (int)phases.size();
  a.nsteps = (int)steps.size();
  a.w = ph.w;
  a.w_lo = (const char*)ph.w + ph.lo_image_bytes;
  a.bias = pc.bias;  // (pc.Npad >= ph.Npad rows)
  a.out = o.ptr;
  a.Do = o.D; a.Ho = o.H; a.Wo = o.W; a.Co = o.Cpad;
  a.Hin = Hin; a.Win = Win;
  a.Q = (int)Q;
  a.Npad = ph.Npad;
  a.relu = 1;
  {
    int n_cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) n_cus = prop.multiProcessorCount;
    h16_tiling(Q, ph.Npad, rows, max_r, h16_balanced() ? n_cus : 0, &a.ntiles, &a.n_big, &a.r_small);
  }
  st.h16_rows = rows;
  st.use_h16 = true;
  return BSMI_OK;
}

// Box-halo launch of one ConvPass stage (conv_box.hip): bf16, 3x3x3, at most 16 output channels.
int Planner::plan_box(const PassSite& p, int ci, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st) {
  st.use_box = false;
  const int* k = p.k[ci];
  if (!box_enabled() || prec != BSMI_PREC_BF16 || k[0] != 3 || k[1] != 3 || k[2] != 3 || !box_supported(p.cout)) return BSMI_OK;
  const bool last = ci == p.nconv - 1;
  const int NB = 1;  // one block of 16 output channels
  const HostWeight& wm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".weight"];
  const HostWeight& bm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".bias"];
  const HostWeight& wr = h->weights[p.prefix + ".residual.0.weight"];
  const HostWeight& br = h->weights[p.prefix + ".residual.0.bias"];
  const int64_t cin_m = wm.shape[1], cin_r = wr.shape[1];
  int crop[3] = {0, 0, 0};
  for (int i = 0; i < p.nconv; ++i)
    for (int d = 0; d < 3; ++d) crop[d] += p.k[i][d] - 1;

  struct Src { int slot, cin_base, creal; };
  std::vector<Src> full, center;
  if (ci == 0) {
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) { full.push_back({s, base, p.cin[s]}); base += p.cin[s]; }
  } else {
    full.push_back({0, 0, p.cout});
  }
  if (last) {
    const int first_slot = ci == 0 ? 0 : 1;
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) { center.push_back({first_slot + s, base, p.cin[s]}); base += p.cin[s]; }
  }
  std::vector<BoxChunk> chunks;
  std::vector<uint32_t> wimg;
  auto chunk_of = [&](const TDesc& t, const int* org, int c0) {
    BoxChunk ck;
    ck.sx = t.Cpad * 2; ck.sy = t.W * ck.sx; ck.sz = t.H * ck.sy;
    ck.base = (uint64_t)(uintptr_t)t.ptr + (uint64_t)org[0] * ck.sz + (uint64_t)org[1] * ck.sy + (uint64_t)org[2] * ck.sx + (uint64_t)c0 * 2;
    ck.D = t.D - org[0]; ck.H = t.H - org[1]; ck.W = t.W - org[2];
    return ck;
  };
  auto put = [&](size_t lane_base, int j, float v) { wimg[lane_base + j / 2] |= (uint32_t)host_f32_to_bf16(v) << (16 * (j & 1)); };
  // FULL chunks: 16 channels x 27 taps, 14 K-steps of (2 taps x 16 channels)
  for (const Src& sr : full) {
    const TDesc& t = slots[sr.slot];
    for (int c0 = 0; c0 < t.Cpad; c0 += 16) {
      chunks.push_back(chunk_of(t, so[sr.slot], c0));
      const size_t w0 = wimg.size();
      wimg.resize(w0 + (size_t)14 * NB * 64 * 4, 0u);
      for (int s = 0; s < 14; ++s)
        for (int b = 0; b < NB; ++b)
          for (int l = 0; l < 64; ++l) {
            const int m = b * 16 + (l & 15), q = l >> 4, tap = 2 * s + (q >> 1);
            if (m >= p.cout || tap >= 27) continue;
            for (int j = 0; j < 8; ++j) {
              const int c = c0 + (q & 1) * 8 + j;
              if (c >= sr.creal) break;
              put(w0 + (((size_t)s * NB + b) * 64 + l) * 4, j, wm.data[((size_t)m * cin_m + (sr.cin_base + c)) * 27 + tap]);
            }
          }
    }
  }
  const int n_full = (int)chunks.size();
  // CENTER chunks: 32 channels of the box's own voxels in the residual source (cropped by half the pass's crop)
  for (const Src& sr : center) {
    const TDesc& t = slots[sr.slot];
    const int org[3] = {so[sr.slot][0] + crop[0] / 2, so[sr.slot][1] + crop[1] / 2, so[sr.slot][2] + crop[2] / 2};
    for (int c0 = 0; c0 < t.Cpad; c0 += 32) {
      chunks.push_back(chunk_of(t, org, c0));
      const size_t w0 = wimg.size();
      wimg.resize(w0 + (size_t)NB * 64 * 4, 0u);
      for (int b = 0; b < NB; ++b)
        for (int l = 0; l < 64; ++l) {
          const int m = b * 16 + (l & 15), q = l >> 4;
          if (m >= p.cout) continue;
          for (int j = 0; j < 8; ++j) {
            const int c = c0 + q * 8 + j;
            if (c >= sr.creal) break;
            put(w0 + ((size_t)b * 64 + l) * 4, j, wr.data[(size_t)m * cin_r + (sr.cin_base + c)]);
          }
        }
    }
  }
  std::vector<float> bias((size_t)16 * NB, 0.f);
  for (int m = 0; m < p.cout; ++m) bias[m] = bm.data[m] + (last ? br.data[m] : 0.f);
  BoxChunk* dchunks = nullptr;
  uint32_t* dw = nullptr;
  float* dbias = nullptr;
  BSMI_HIP(hipMalloc((void**)&dchunks, chunks.size() * sizeof(BoxChunk)));
  plan->allocs.push_back(dchunks);
  BSMI_HIP(hipMalloc((void**)&dw, wimg.size() * 4));
  plan->allocs.push_back(dw);
  BSMI_HIP(hipMalloc((void**)&dbias, bias.size() * 4));
  plan->allocs.push_back(dbias);
  BSMI_HIP(hipMemcpy(dchunks, chunks.data(), chunks.size() * sizeof(BoxChunk), hipMemcpyHostToDevice));
  BSMI_HIP(hipMemcpy(dw, wimg.data(), wimg.size() * 4, hipMemcpyHostToDevice));
  BSMI_HIP(hipMemcpy(dbias, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
  st.box.chunks = dchunks;
  st.box.n_full = n_full;
  st.box.n_center = (int)chunks.size() - n_full;
  st.box.w = dw;
  st.box.bias = dbias;
  st.box.out = (uint16_t*)o.ptr;
  st.box.Do = o.D; st.box.Ho = o.H; st.box.Wo = o.W; st.box.Co = o.Cpad;
  st.use_box = true;
  return BSMI_OK;
}

// One ConvPass (reference unet.py:63-76).  in[s] with per-slot origin org[s]; `sp` is the
// logical input extent (the extent of the concatenated, cropped input).
int Planner::pass(PassSite& p, const TDesc* in, const int (*org)[3], const int sp_in[3], TDesc& out) {
  int sp[3] = {sp_in[0], sp_in[1], sp_in[2]};
  TDesc cur;
  for (int ci = 0; ci < p.nconv; ++ci) {
    const bool last = ci == p.nconv - 1;
    TDesc o;
    o.C = p.cout;
    o.D = sp[0] - (p.k[ci][0] - 1);
    o.H = sp[1] - (p.k[ci][1] - 1);
    o.W = sp[2] - (p.k[ci][2] - 1);
    if (o.D <= 0 || o.H <= 0 || o.W <= 0)
      BSMI_FAIL(BSMI_ERR_INVALID, "%s: input extent (%d,%d,%d) too small for kernel (%d,%d,%d)",
                p.prefix.c_str(), sp[0], sp[1], sp[2], p.k[ci][0], p.k[ci][1], p.k[ci][2]);
    int rc = alloc(o);
    if (rc) return rc;

    // tensor slots of this launch and their origins
    TDesc slots[kMaxConvTensors];
    int so[kMaxConvTensors][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int nsl = 0;
    if (ci == 0) {
      for (int s = 0; s < p.nslots; ++s) {
        slots[nsl] = in[s];
        for (int d = 0; d < 3; ++d) so[nsl][d] = org[s][d];
        ++nsl;
      }
    } else {
      slots[nsl++] = cur;
      if (last)
        for (int s = 0; s < p.nslots; ++s) {
          slots[nsl] = in[s];
          for (int d = 0; d < 3; ++d) so[nsl][d] = org[s][d];
          ++nsl;
        }
    }

    // flops: 2 * M * Cout * K_real
    const double M = (double)o.D * o.H * o.W;
    double kreal = 0;
    {
      std::vector<PackEntry> ents;
      build_entries(p, ci, prec, ents);
      for (auto& e : ents) if (!e.dummy) kreal += std::max(0, std::min(e.creal - e.c0, sube(prec)));
    }
    plan->flops += 2.0 * M * p.cout * kreal;

    if (!dry) {
      PackedConv& pc = p.packed[prec][ci];
      PlanStep st;
      st.type = PlanStep::CONV;
      st.tile = pc.tile;
      ConvArgs& a = st.conv;
      memset(&a, 0, sizeof a);
      const int KS = pc.ks;
      std::vector<KStep> ks(pc.entries.size() / kUnitsPerStep * KS);
      const int64_t es = esize(prec) * (prec == BSMI_PREC_BF16X3 ? 2 : 1);  // bytes per channel of a row: (hi, lo) interleaved
      for (int sl = 0; sl < kMaxConvTensors; ++sl) {
        const TDesc& t = slots[sl < nsl ? sl : 0];
        a.t[sl].base = (uint64_t)(uintptr_t)t.ptr;
        a.t[sl].sz = (int32_t)((int64_t)t.H * t.W * t.Cpad * es);
        a.t[sl].sy = (int32_t)((int64_t)t.W * t.Cpad * es);
        a.t[sl].sx = (int32_t)((int64_t)t.Cpad * es);
      }
      for (size_t s = 0; s < ks.size() / KS; ++s) {
        const int slot = pc.entries[kUnitsPerStep * s].slot;
        const TDesc& t = slots[slot];
        KStep k;
        memset(&k, 0, sizeof k);
        k.tensor = slot;
        for (int j = 0; j < kUnitsPerStep; ++j) {
          const PackEntry& e = pc.entries[kUnitsPerStep * s + j];
          if (e.dummy) continue;
          const int64_t off = ((((int64_t)(e.dz + so[slot][0]) * t.H) + (e.dy + so[slot][1])) * t.W +
                               (e.dx + so[slot][2])) * t.Cpad + e.c0;
          k.delta[j] = (int32_t)(off * es);
        }
        ks[s * KS] = k;
        if (KS == 3) {
          KStep lo = k;  // the same taps of the lo plane (a padding unit stays at offset 0: it meets zero weights)
          for (int j = 0; j < kUnitsPerStep; ++j)
            if (!pc.entries[kUnitsPerStep * s + j].dummy) lo.delta[j] = (int32_t)(k.delta[j] + (int64_t)t.lo_off);
          ks[s * KS + 1] = lo;
          ks[s * KS + 2] = k;
        }
      }
      if ((rc = upload_ksteps(plan, ks, a))) return rc;
      a.w = pc.w;
      a.w_lo = pc.lo_image_bytes ? (const char*)pc.w + pc.lo_image_bytes : nullptr;
      a.bias = pc.bias;
      a.out = o.ptr;
      a.Do = o.D; a.Ho = o.H; a.Wo = o.W; a.Co = o.Cpad;
      a.M = o.D * o.H * o.W;
      a.Npad = pc.Npad;
      a.relu = 1;  // trunk activation is ReLU (model.py passes activation default "ReLU")
      st.flops = 2.0 * M * p.cout * kreal;
      {
        const double x3 = prec == BSMI_PREC_BF16X3 ? 3.0 : 1.0;
        const double kstep = (double)kUnitsPerStep * sube(prec);   // channels x taps of one K-step
        st.exec_flops = 2.0 * (double)round_up(a.M, 256) * pc.Npad * ((double)(ks.size() / KS) * kstep) * x3;
      }
      st.site = &p;
      st.ci = ci;
      st.nsl = nsl;
      for (int sl = 0; sl < nsl; ++sl) {
        st.slots[sl] = slots[sl];
        for (int d = 0; d < 3; ++d) st.so[sl][d] = so[sl][d];
      }
      st.out = o;
      rc = plan_rh(p, ci, pc, slots, so, o, st);
      if (rc) return rc;
      rc = plan_box(p, ci, slots, so, o, st);
      if (rc) return rc;
      rc = plan_wino(p, ci, pc, slots, so, nsl, o, st);
      if (rc) return rc;
      if (!st.use_wino && !st.use_box) {
        rc = plan_h16(p, ci, pc, slots, so, o, st);
        if (rc) return rc;
      }
      if (getenv("BSMI_PLAN_DEBUG"))
        fprintf(stderr, "[bsmi plan] %s conv %d: out (%d,%d,%d)x%d tile BN=%d K-steps %d %s\n", p.prefix.c_str(), ci, o.D, o.H, o.W,
                p.cout, tile_bn(st.tile), st.use_wino ? st.wino_gemm.nsteps : a.nsteps,
                st.use_wino ? (st.wino_in.m == 4 ? "winograd F(4x4,3x3)" : "winograd F(2x2,3x3)") : st.use_h16 ? "halo-resident" : st.use_box ? "box-halo" : st.use_rh ? "raster-halo" : "gather");
      plan->steps.push_back(st);
    }
    cur = o;
    sp[0] = o.D; sp[1] = o.H; sp[2] = o.W;
  }
  out = cur;
  return BSMI_OK;
}

int Planner::rec(int level, const TDesc& f_in, TDesc& f_out) {
  const int i = h->nl - level - 1;
  TDesc f_left;
  const int org0[1][3] = {{0, 0, 0}};
  const int sp[3] = {f_in.D, f_in.H, f_in.W};
  int rc = pass(h->l_conv[i], &f_in, org0, sp, f_left);
  if (rc) return rc;
  if (level == 0) {
    f_out = f_left;
    return BSMI_OK;
  }
  const int* f = h->cfg.downsample_factors[i];
  const int dims[3] = {f_left.D, f_left.H, f_left.W};
  for (int d = 2; d >= 0; --d)
    if (dims[d] % f[d] != 0)
      BSMI_FAIL(BSMI_ERR_INVALID,
                "Can not downsample shape (%d, %d, %d) with factor (%d, %d, %d), mismatch in spatial dimension %d",
                dims[0], dims[1], dims[2], f[0], f[1], f[2], d);
  TDesc g_in;
  g_in.C = f_left.C; g_in.D = f_left.D / f[0]; g_in.H = f_left.H / f[1]; g_in.W = f_left.W / f[2];
  rc = alloc(g_in);
  if (rc) return rc;
  if (!dry) {
    PlanStep st;
    st.type = PlanStep::POOL;
    st.in = f_left; st.out = g_in;
    for (int d = 0; d < 3; ++d) st.f[d] = f[d];
    // Fused pooling (BSMI_POOL_FUSE=0: off): behind an F(4x4) stage a (1,2,2) pool of even extents is stored by the stage's
    // output transform, whose threads hold whole 4 x 4 tiles (WinoOutArgs::pool) -- the launch that re-read the tensor just
    // written (0.40 GB for the 300-channel one of the 128^3 block) falls away.  Same bits; the full-resolution tensor is
    // still written, the skip connection reads it.
    PlanStep& prod = plan->steps.back();
    if (pool_fuse_enabled() && prec == BSMI_PREC_BF16X3 && f[0] == 1 && f[1] == 2 && f[2] == 2 && prod.type == PlanStep::CONV && prod.use_wino &&
        prod.wino_out.m == 4 && !prod.wino_out.low && !prod.wino_out.wz && prod.wino_out.out == f_left.ptr && !(f_left.H & 1) && !(f_left.W & 1)) {
      prod.wino_out.pool = g_in.ptr;
      st.pool_fused = true;
    }
    plan->steps.push_back(st);
  }
  TDesc g_out;
  rc = rec(level - 1, g_in, g_out);
  if (rc) return rc;

  // Upsample.forward (unet.py:215-223): upsample, crop_to_factor, crop skip, concat
  PassSite& rp = h->r_conv[i];
  const int up[3] = {g_out.D * f[0], g_out.H * f[1], g_out.W * f[2]};
  int conv_crop[3] = {0, 0, 0};
  for (int c = 0; c < rp.nconv; ++c)
    for (int d = 0; d < 3; ++d) conv_crop[d] += rp.k[c][d] - 1;
  int target[3];
  for (int d = 0; d < 3; ++d) {
    const int cf = h->crop_factor[i][d];
    const int n = (int)std::floor((double)(up[d] - conv_crop[d]) / cf);
    target[d] = n * cf + conv_crop[d];
    if (target[d] != up[d] && target[d] <= conv_crop[d])
      BSMI_FAIL(BSMI_ERR_INVALID,
                "Feature map with shape (%d, %d, %d) is too small to ensure translation equivariance",
                up[0], up[1], up[2]);
  }
  TDesc g_c;
  g_c.C = g_out.C; g_c.D = target[0]; g_c.H = target[1]; g_c.W = target[2];
  rc = alloc(g_c);
  if (rc) return rc;
  int so[2][3];
  for (int d = 0; d < 3; ++d) {
    so[0][d] = (dims[d] - target[d]) / 2;
    so[1][d] = 0;
    if (dims[d] < target[d])
      BSMI_FAIL(BSMI_ERR_INVALID, "skip connection (%d,%d,%d) smaller than upsampled map (%d,%d,%d)",
                dims[0], dims[1], dims[2], target[0], target[1], target[2]);
  }
  // Fused upsampling (BSMI_FUSE_UP=0: off): when the first and the last stage of the ConvPass both run in Winograd form, they
  // read the map below the upsampling and interpolate on the fly -- the first stage's input transform, and the last stage's
  // residual branch as a 1x1x1 convolution BELOW the upsampling (it commutes with the per-channel interpolation) whose sums
  // the output transform interpolates.  The upsampled map (1.3 GB for the 1500-channel one of the 128^3 block) is then
  // neither written nor read: 0.54 ms of upsampling, 1 GB of transform reads and four fifths of the residual GEMM saved.
  UpFuse uf;
  bool fuse = false;
  if (!dry && prec == BSMI_PREC_BF16X3 && f[0] == 1 && f[1] == 2 && f[2] == 2 && rp.nslots == 2 && rp.wino[0].ready &&
      rp.wino[rp.nconv - 1].ready && !rp.wino[rp.nconv - 1].res_part[1].empty() && g_out.ptr) {
    fuse = fuse_up_enabled();
    int sp[3] = {target[0], target[1], target[2]};
    for (int c = 0; c < rp.nconv && fuse; ++c) {
      for (int d = 0; d < 3; ++d) sp[d] -= rp.k[c][d] - 1;
      const int wm = rp.wino[c].m;
      if ((c == 0 || c == rp.nconv - 1) && ((wm == 2 && ((sp[1] & 1) || (sp[2] & 1))) || sp[0] <= 0 || sp[1] <= 0 || sp[2] <= 0)) fuse = false;
      if ((c == 0 || c == rp.nconv - 1) && (size_t)(sp[0] + 2) * ((sp[1] + wm - 1) / wm) * ((sp[2] + wm - 1) / wm) * rp.wino[c].Cv * 4 >= ((size_t)1 << 31)) fuse = false;
    }
  }
  if (!dry) {
    PlanStep st;
    st.type = PlanStep::UP;
    st.in = g_out; st.out = g_c;
    for (int d = 0; d < 3; ++d) { st.f[d] = f[d]; st.o[d] = (up[d] - target[d]) / 2; }
    st.skip = fuse;
    plan->steps.push_back(st);
  }
  if (fuse) {
    uf.low = g_out;
    for (int d = 0; d < 3; ++d) { uf.f[d] = f[d]; uf.o[d] = (up[d] - target[d]) / 2; }
    fuse_up = &uf;
    if (getenv("BSMI_PLAN_DEBUG")) fprintf(stderr, "[bsmi plan] %s: upsampling fused into the Winograd stages\n", rp.prefix.c_str());
  }
  const TDesc ins[2] = {f_left, g_c};
  rc = pass(rp, ins, so, target, f_out);
  fuse_up = nullptr;
  return rc;
}

int Planner::run(const int64_t in_shape[3]) {
  TDesc x;
  x.C = h->cfg.in_channels; x.D = (int)in_shape[0]; x.H = (int)in_shape[1]; x.W = (int)in_shape[2];
  int rc = alloc(x);
  if (rc) return rc;
  if (!dry) {
    PlanStep st;
    st.type = PlanStep::INPUT;
    st.out = x;
    plan->steps.push_back(st);
  }
  TDesc z;
  rc = rec(h->nl - 1, x, z);
  if (rc) return rc;
  plan->out_shape[0] = z.D; plan->out_shape[1] = z.H; plan->out_shape[2] = z.W;
  for (size_t hd = 0; hd < h->heads.size(); ++hd) {
    plan->flops += 2.0 * 2.0 * (double)z.D * z.H * z.W * h->heads[hd].cin * h->heads[hd].cout;
    if (!dry) {
      PlanStep st;
      st.type = PlanStep::HEAD;
      st.in = z;
      st.head = (int)hd;
      st.flops = 2.0 * 2.0 * (double)z.D * z.H * z.W * h->heads[hd].cin * h->heads[hd].cout;
      plan->steps.push_back(st);
    }
  }
  return BSMI_OK;
}

void free_plan(Plan* p) {
for (void* a : p->allocs) (void)hipFree(a);
p->allocs.clear();
for (auto* sets : {&p->inflight, &p->spare})
  for (auto& set : *sets)
    for (hipEvent_t e : set) (void)hipEventDestroy(e);
p->inflight.clear();
p->spare.clear();
p->events.clear();
}

int get_plan(bsmi_unet* h, int precision, const int64_t in_shape[3], Plan** out) {
  const std::vector<int64_t> key = {precision, in_shape[0], in_shape[1], in_shape[2]};
  auto it = h->plans.find(key);
  if (it == h->plans.end()) {
    std::unique_ptr<Plan> plan(new Plan);
    plan->prec = precision;
    Planner pl{h, precision, plan.get(), false};
    const int rc = pl.run(in_shape);
    if (rc) {
      free_plan(plan.get());
      return rc;
    }
    const std::vector<PlanStep>& ps = plan->steps;
    const bool fp_ready = precision == BSMI_PREC_BF16 ? h->first_pass.ready : precision == BSMI_PREC_BF16X3 && h->first_pass_x3.ready;
    plan->fused_first = fp_ready && first_pass_eligible(h) && ps.size() > 3 &&
                        ps[0].type == PlanStep::INPUT && ps[1].type == PlanStep::CONV && ps[2].type == PlanStep::CONV &&
                        ps[1].site == &h->l_conv[0] && ps[2].site == &h->l_conv[0] && ps[2].out.Cpad == 16;
    if (plan->fused_first && plan->steps[3].type == PlanStep::POOL && plan->steps[3].pool_fused) {
      // step 2 runs inside first_pass and not as the Winograd stage that would have stored the pooled tensor
      plan->steps[3].pool_fused = false;
      plan->steps[2].wino_out.pool = nullptr;
    }
    // the planner's uploads and fills (hipMemcpy / hipMemsetAsync on the null stream) before any launch on a caller's non-blocking stream
    BSMI_HIP(hipDeviceSynchronize());
    it = h->plans.emplace(key, std::move(plan)).first;
  }
  *out = it->second.get();
  return BSMI_OK;
}

int check_shape_arg(const int64_t s[3]) {
  for (int d = 0; d < 3; ++d)
    if (s[d] <= 0 || s[d] > 4096) BSMI_FAIL(BSMI_ERR_INVALID, "bad input shape (%lld,%lld,%lld)", (long long)s[0], (long long)s[1], (long long)s[2]);
  return BSMI_OK;
}

int dry_plan(bsmi_unet* h, const int64_t in_shape[3], Plan& plan) {
  int rc = check_shape_arg(in_shape);
  if (rc) return rc;
  Planner pl{h, BSMI_PREC_BF16, &plan, true};
  return pl.run(in_shape);
}

}  // namespace bsmi

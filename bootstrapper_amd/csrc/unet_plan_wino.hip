// The Winograd form of a ConvPass stage (Planner::plan_wino): one function decides and allocates, one function per launch
// builds its arguments -- input transform, batched GEMM, the nine-tap launch below a fused upsampling, the low-resolution
// residual, the residual, output transform.
#include <cstring>

#include "unet_plan.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

namespace {

// a raw launch of the fused split-bf16 kernel, one GEMM: f32 sums as they are (no bias, no ReLU) from the (hi, lo) images at `w`
void raw_gemm(ConvArgs& a, const void* w, size_t lo_image_bytes, int Npad) {
  a.w = w;
  a.w_lo = (const char*)w + lo_image_bytes;
  a.Npad = Npad;
  a.relu = 0;
  a.raw = 1;
  a.nbatch = 0;
  a.a_batch = a.w_batch = 0;
}

// One Winograd stage while it is planned: the stage, its geometry, the buffers its launches hand to one another, and one
// function per launch.
struct WinoStage {
  Plan* plan;
  const UpFuse* fuse_up;
  const PassSite& p;
  int ci;
  const PackedConv& pc;
  const PackedWino& pw;
  const TDesc* slots;
  const int (*so)[3];
  const TDesc& o;
  PlanStep& st;
  bool below;  // the upsampled source leaves the Winograd form (PackedWino::below_*); V holds the skip connection alone
  bool cut;    // the residual branch in two parts: the skip connection here, the upsampled map below the upsampling
  bool wz;     // F(2,3) along z as well (PackedWino::wz): Dv = pairs of output planes, the GEMM a 1x1x1 convolution of V[36 e + b]
  int wm, nbatch, Dv, Ty, Tx, Cv;
  size_t vbatch, Mrows;  // bytes of one batch of V, rows of one batch of the GEMM
  void *V = nullptr, *Mbuf = nullptr, *addend = nullptr, *low = nullptr, *Ybuf = nullptr;
  size_t Mbelow = 0;
  int low_off[3] = {0, 0, 0}, below_off[3] = {0, 0, 0};

  int input_transform() {
    WinoInArgs& wi = st.wino_in;
    memset(&wi, 0, sizeof wi);
    const int nsrc = below ? 1 : ci == 0 ? p.nslots : 1;
    int cv0 = 0;
    for (int q = 0; q < nsrc; ++q) {
      const TDesc& t = slots[q];
      wi.src[q] = t.ptr;
      wi.H[q] = t.H; wi.W[q] = t.W; wi.Cpad[q] = t.Cpad;
      wi.oz[q] = so[q][0]; wi.oy[q] = so[q][1]; wi.ox[q] = so[q][2];
      wi.cv0[q] = cv0;
      cv0 += t.Cpad;
      if (fuse_up && ci == 0 && q == 1) {  // the upsampled map: read below the upsampling
        if (fuse_up->low.Cpad != t.Cpad) BSMI_FAIL(BSMI_ERR_STATE, "%s: fused upsampling with a different channel padding", p.prefix.c_str());
        wi.src[q] = fuse_up->low.ptr;
        wi.H[q] = fuse_up->low.H; wi.W[q] = fuse_up->low.W;
        wi.oz[q] += fuse_up->o[0]; wi.oy[q] += fuse_up->o[1]; wi.ox[q] += fuse_up->o[2];
        wi.upf[q] = fuse_up->f[1];
      }
    }
    if (cv0 != Cv) BSMI_FAIL(BSMI_ERR_STATE, "%s conv %d: winograd channel layout %d != %d", p.prefix.c_str(), ci, cv0, Cv);
    wi.nsrc = nsrc;
    wi.V = V;
    wi.Dv = Dv; wi.Ty = Ty; wi.Tx = Tx; wi.Cv = Cv;
    wi.m = wm;
    wi.wz = wz ? 1 : 0;
    wi.Dz = o.D + 2;
    return BSMI_OK;
  }

  // the batched GEMMs: a (3,1,1) convolution of V[b] with U[b]; wz: a 1x1x1 convolution of V[36 e + b] over the pairs (its
  // units carry kz = 0: the K-step list is channels only)
  int batched_gemm() {
    const std::vector<WinoUnit>& units = below ? pw.skip_units : pw.units;
    ConvArgs& g = st.wino_gemm;
    memset(&g, 0, sizeof g);
    set_strides(g, V, Ty, Tx, Cv, 4);
    std::vector<KStep> ks(units.size() / kUnitsPerStep);
    for (size_t s = 0; s < ks.size(); ++s) {
      KStep k;
      memset(&k, 0, sizeof k);
      for (int j = 0; j < kUnitsPerStep; ++j) {
        const WinoUnit& u = units[kUnitsPerStep * s + j];
        if (!u.dummy) k.delta[j] = (int32_t)(((int64_t)u.kz * Ty * Tx * Cv + u.vc0) * 4);
      }
      ks[s] = k;
    }
    const int rc = upload_ksteps(plan, ks, g);
    if (rc) return rc;
    raw_gemm(g, below ? pw.skip_w : pw.w, below ? pw.skip_lo_image_bytes : pw.lo_image_bytes, pw.Npad);
    g.bias = pc.bias;
    g.out = Mbuf;
    g.Do = wz ? Dv : o.D; g.Ho = Ty; g.Wo = Tx; g.Co = o.Cpad;
    g.M = (int)Mrows;
    g.nbatch = nbatch;
    g.a_batch = (int64_t)vbatch;
    g.w_batch = (int64_t)(below ? pw.skip_batch_bytes : pw.batch_bytes);
    return BSMI_OK;
  }

  // below-up: Y[tap][z][i][j][n] = sum_{kz, c} W[n][c][kz][tap] L[z + kz + oz][i][j][c] over whole planes of the low-resolution
  // tensor L, one raw launch: the nine taps as nine batches over the same rows, or side by side as columns (below_dense)
  int below_up() {
    const TDesc& lt = fuse_up->low;
    for (int d = 0; d < 3; ++d) below_off[d] = so[1][d] + fuse_up->o[d];
    if (fuse_up->f[1] != 2 || fuse_up->f[2] != 2 || lt.Cpad != slots[1].Cpad || below_off[0] < 0 || below_off[0] + o.D + 2 > lt.D || below_off[1] < 0 ||
        below_off[2] < 0 || below_off[1] + o.H + 2 > 2 * lt.H || below_off[2] + o.W + 2 > 2 * lt.W)
      BSMI_FAIL(BSMI_ERR_STATE, "%s: the low-resolution tensor does not cover the stage's input", p.prefix.c_str());
    Mbelow = (size_t)o.D * lt.H * lt.W;
    const size_t ybytes = 9 * Mbelow * o.Cpad * sizeof(float);
    if (Mbelow * 9 >= ((size_t)1 << 31)) BSMI_FAIL(BSMI_ERR_STATE, "%s: too many rows of sums below the upsampling", p.prefix.c_str());
    BSMI_HIP(hipMalloc(&Ybuf, ybytes));
    plan->allocs.push_back(Ybuf);
    plan->bytes += ybytes;
    ConvArgs& r = st.wino_below;
    memset(&r, 0, sizeof r);
    set_strides(r, lt.ptr, lt.H, lt.W, lt.Cpad, 4);
    std::vector<KStep> ks(pw.below_units.size() / kUnitsPerStep);
    for (size_t s = 0; s < ks.size(); ++s) {
      KStep k;
      memset(&k, 0, sizeof k);
      for (int j = 0; j < kUnitsPerStep; ++j) {
        const WinoUnit& u = pw.below_units[kUnitsPerStep * s + j];
        if (!u.dummy) k.delta[j] = (int32_t)(((int64_t)(u.kz + below_off[0]) * lt.H * lt.W * lt.Cpad + u.vc0) * 4);
      }
      ks[s] = k;
    }
    const int rc = upload_ksteps(plan, ks, r);
    if (rc) return rc;
    raw_gemm(r, pw.below_w, pw.below_lo_image_bytes, pw.below_Npad);
    r.bias = pc.bias;
    r.out = Ybuf;
    r.Do = o.D; r.Ho = lt.H; r.Wo = lt.W;
    r.Co = pw.below_dense ? 9 * o.Cpad : o.Cpad;
    r.M = (int)Mbelow;
    r.nbatch = pw.below_dense ? 0 : 9;
    r.w_batch = (int64_t)pw.below_batch_bytes;
    st.below_tile = pw.below_tile;
    st.wino_has_below = true;
    return BSMI_OK;
  }

  // the upsampled map's part of a cut residual branch: a 1x1x1 convolution of the low-resolution tensor itself, whose sums the
  // output transform interpolates
  int residual_low() {
    const TDesc& g = fuse_up->low;
    const size_t Mlow = (size_t)g.D * g.H * g.W;
    BSMI_HIP(hipMalloc(&low, Mlow * o.Cpad * sizeof(float)));
    plan->allocs.push_back(low);
    plan->bytes += Mlow * o.Cpad * sizeof(float);
    ConvArgs& r = st.wino_res_low;
    memset(&r, 0, sizeof r);
    set_strides(r, g.ptr, g.H, g.W, g.Cpad, 4);
    const std::vector<PackEntry>& ents = pw.res_part[1];
    std::vector<KStep> ks(ents.size() / kUnitsPerStep);
    int up_slot = -1;
    for (size_t s = 0; s < ks.size(); ++s) {
      KStep k;
      memset(&k, 0, sizeof k);
      for (int j = 0; j < kUnitsPerStep; ++j) {
        const PackEntry& e = ents[kUnitsPerStep * s + j];
        if (e.dummy) continue;
        k.delta[j] = (int32_t)((int64_t)e.c0 * 4);  // a 1x1x1 convolution of the low-resolution tensor itself: no spatial offset here
        up_slot = e.slot;
        low_off[0] = e.dz; low_off[1] = e.dy; low_off[2] = e.dx;  // the branch's crop: applied by the output transform
      }
      ks[s] = k;
    }
    if (up_slot < 0) BSMI_FAIL(BSMI_ERR_STATE, "%s: empty low-resolution residual", p.prefix.c_str());
    for (int d = 0; d < 3; ++d) low_off[d] += so[up_slot][d] + fuse_up->o[d];
    const int rc = upload_ksteps(plan, ks, r);
    if (rc) return rc;
    raw_gemm(r, pw.res_part_w[1], pw.res_part_lo[1], pw.Npad);
    r.bias = pc.bias;
    r.out = low;
    r.Do = g.D; r.Ho = g.H; r.Wo = g.W; r.Co = o.Cpad;
    r.M = (int)Mlow;
    st.wino_has_res_low = true;
    return BSMI_OK;
  }

  // the residual branch at full resolution (of a cut branch: the skip connection's part): its K-steps alone, raw sums the output
  // transform adds
  int residual() {
    const std::vector<PackEntry>& res_entries = cut ? pw.res_part[0] : pw.res_entries;
    BSMI_HIP(hipMalloc(&addend, (size_t)o.D * o.H * o.W * o.Cpad * sizeof(float)));
    plan->allocs.push_back(addend);
    plan->bytes += (size_t)o.D * o.H * o.W * o.Cpad * sizeof(float);
    ConvArgs& r = st.wino_res;
    r = st.conv;  // the direct launch's source tensors and output geometry
    std::vector<KStep> ks(res_entries.size() / kUnitsPerStep);
    for (size_t s = 0; s < ks.size(); ++s) {
      KStep k;
      memset(&k, 0, sizeof k);
      const PackEntry& e0 = res_entries[kUnitsPerStep * s];
      k.tensor = e0.dummy ? 0 : e0.slot;
      for (int j = 0; j < kUnitsPerStep; ++j) {
        const PackEntry& e = res_entries[kUnitsPerStep * s + j];
        if (e.dummy) continue;
        const TDesc& t = slots[e.slot];
        const int64_t off = ((((int64_t)(e.dz + so[e.slot][0]) * t.H) + (e.dy + so[e.slot][1])) * t.W + (e.dx + so[e.slot][2])) * t.Cpad + e.c0;
        k.delta[j] = (int32_t)(off * 4);
      }
      ks[s] = k;
    }
    const int rc = upload_ksteps(plan, ks, r);
    if (rc) return rc;
    raw_gemm(r, cut ? pw.res_part_w[0] : pw.res_w, cut ? pw.res_part_lo[0] : pw.res_lo_image_bytes, pw.Npad);
    r.out = addend;
    return BSMI_OK;
  }

  // the output transform (bias, residual, ReLU, (hi, lo) pairs), and what the stage's launches give the matrix pipe
  void output_transform(int prec) {
    WinoOutArgs& wo = st.wino_out;
    memset(&wo, 0, sizeof wo);
    wo.M = (const float*)Mbuf;
    wo.addend = (const float*)addend;
    if (cut) {
      wo.low = (const float*)low;
      wo.lD = fuse_up->low.D; wo.lH = fuse_up->low.H; wo.lW = fuse_up->low.W;
      wo.lf = fuse_up->f[1];
      wo.loz = low_off[0]; wo.loy = low_off[1]; wo.lox = low_off[2];
    }
    if (below) {
      wo.below = (const float*)Ybuf;
      wo.btap = pw.below_dense ? (int64_t)o.Cpad : (int64_t)Mbelow * o.Cpad;
      wo.brow = pw.below_dense ? 9 * o.Cpad : o.Cpad;
      wo.boy = below_off[1]; wo.box = below_off[2];
      wo.lD = fuse_up->low.D; wo.lH = fuse_up->low.H; wo.lW = fuse_up->low.W;
      wo.lf = fuse_up->f[1];
    }
    wo.bias = pc.bias;
    wo.out = o.ptr;
    wo.Do = o.D; wo.Ty = Ty; wo.Tx = Tx; wo.Co = o.Cpad;
    wo.m = wm; wo.Ho = o.H; wo.Wo = o.W;
    wo.relu = 1;
    wo.wz = wz ? 1 : 0;
    // (nbatch, Mrows and the K-step count are the form's own: 144 batches of ceil(Do / 2) Ty Tx rows over K = Cv in the wz form)
    const double kstep = (double)kUnitsPerStep * sube(prec);
    st.exec_flops = 2.0 * (double)round_up((int)Mrows, 256) * pw.Npad * ((double)st.wino_gemm.nsteps * kstep) * nbatch * 3.0;
    if (st.wino_has_res) st.exec_flops += 2.0 * (double)round_up(st.wino_res.M, 256) * pw.Npad * ((double)st.wino_res.nsteps * kstep) * 3.0;
    if (st.wino_has_res_low) st.exec_flops += 2.0 * (double)round_up(st.wino_res_low.M, 256) * pw.Npad * ((double)st.wino_res_low.nsteps * kstep) * 3.0;
    if (st.wino_has_below)
      st.exec_flops += 2.0 * (double)round_up(st.wino_below.M, 256) * pw.below_Npad * (pw.below_dense ? 1 : 9) * ((double)st.wino_below.nsteps * kstep) * 3.0;
  }
};

}  // namespace

// Winograd form of one 3x3x3 stage (wino.hip): the layer's sources are transformed into V (16 batches), one batched launch
// of the fused split-bf16 kernel multiplies them with the transformed weights into raw f32 sums, the residual branch of a
// last stage runs as a short launch of its own, and the output transform finishes (bias, residual, ReLU, (hi, lo) pairs).
int Planner::plan_wino(PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], int nsl, const TDesc& o, PlanStep& st) {
  st.use_wino = false;
  const PackedWino& pw = p.wino[ci];
  const bool wants_fused = fuse_up && (ci == 0 || ci == p.nconv - 1);
  if (pw.fused_only && !fuse_up) return BSMI_OK;  // the upsampling of this pass is not fused: the stage keeps its other form
  const bool wz = pw.wz;
  const int wm = pw.m, nbatch = wino_batches(wm) * (wz ? kWinoZ : 1);
  if (wz && (wm != 4 || wants_fused)) BSMI_FAIL(BSMI_ERR_STATE, "%s conv %d: packed for the z transform, but planned behind a fused upsampling", p.prefix.c_str(), ci);
  if (prec != BSMI_PREC_BF16X3 || !pw.ready || (wm == 2 && ((o.H & 1) || (o.W & 1))) || st.use_box || st.use_rh) {
    if (wants_fused) BSMI_FAIL(BSMI_ERR_STATE, "%s conv %d: the upsampling was fused into this stage, which cannot take the Winograd form", p.prefix.c_str(), ci);
    return BSMI_OK;
  }
  // below-up: the upsampled source leaves the Winograd form (PackedWino::below_*); V holds the skip connection alone
  const bool below = fuse_up && ci == 0 && pw.below_ready && wm == 4 && nsl == 2;
  const int Dv = wz ? (o.D + 1) / 2 : o.D + 2, Ty = (o.H + wm - 1) / wm, Tx = (o.W + wm - 1) / wm, Cv = below ? pw.skip_Cv : pw.Cv;   // F(4x4): the last tiles may overhang
  const size_t vbatch = (size_t)Dv * Ty * Tx * Cv * 4;  // bytes of one batch of V: (hi, lo) pairs
  if (vbatch >= ((size_t)1 << 31)) {                     // 31-bit byte offsets inside a batch
    if (wants_fused) BSMI_FAIL(BSMI_ERR_STATE, "%s conv %d: fused upsampling, but the transformed input is too large", p.prefix.c_str(), ci);
    return BSMI_OK;
  }
  const size_t Mrows = (size_t)(wz ? Dv : o.D) * Ty * Tx;
  if (Mrows >= ((size_t)1 << 31)) BSMI_FAIL(BSMI_ERR_STATE, "%s conv %d: too many rows in a batch of the transform-domain GEMM", p.prefix.c_str(), ci);
  // residual branch
  const bool cut = fuse_up && ci == p.nconv - 1;  // the branch in two parts: the skip connection here, the upsampled map below the upsampling
  WinoStage w{plan, fuse_up, p, ci, pc, pw, slots, so, o, st, below, cut, wz, wm, nbatch, Dv, Ty, Tx, Cv, vbatch, Mrows};
  BSMI_HIP(hipMalloc(&w.V, (size_t)nbatch * vbatch + 4096));
  plan->allocs.push_back(w.V);
  BSMI_HIP(hipMalloc(&w.Mbuf, (size_t)nbatch * Mrows * o.Cpad * sizeof(float)));
  plan->allocs.push_back(w.Mbuf);
  plan->bytes += nbatch * (vbatch + Mrows * o.Cpad * sizeof(float));
  int rc = w.input_transform();
  if (rc || (rc = w.batched_gemm())) return rc;
  st.wino_has_below = false;
  if (below && (rc = w.below_up())) return rc;
  if (cut && (pw.res_part[0].empty() || pw.res_part[1].empty())) BSMI_FAIL(BSMI_ERR_STATE, "%s: fused upsampling without a cut residual branch", p.prefix.c_str());
  st.wino_has_res = !(cut ? pw.res_part[0] : pw.res_entries).empty();
  st.wino_has_res_low = false;
  if (cut && (rc = w.residual_low())) return rc;
  if (st.wino_has_res && (rc = w.residual())) return rc;
  w.output_transform(prec);
  st.tile = pw.tile;
  st.use_wino = true;
  return BSMI_OK;
}

}  // namespace bsmi

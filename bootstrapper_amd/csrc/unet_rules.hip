// Form rules of the U-Net engine: which stage takes which kernel form, and the BSMI_* switches that override the rules for tests
// and A/B runs.  Every switch is read once per process; the measurements behind a rule are recorded beside it.  The packing
// (unet_pack.hip) asks these rules which images to build, the planner (unet_plan.hip, unet_plan_wino.hip) which launches.
#include <cstdlib>

#include "unet_internal.h"

namespace bsmi {

// Which form of the split mode a layer takes: the fused kernel (conv_x3_body) or three listed K-steps through the bf16
// kernels.  BSMI_X3_FUSED (dev / tests): 0 = listed form everywhere, 1 (default) / 2 = fused wherever the 8-wave kernels
// run, 3 = fused except on 256 x 320 tiles (the two forms side by side in one forward).
static int x3_fused_mode() {
  static const int m = [] { const char* e = getenv("BSMI_X3_FUSED"); return e ? atoi(e) : 1; }();
  return m;
}
bool x3_fused_for(TileCfg tile) {
  if (!two_waves_per_simd()) return false;  // BSMI_WAVES8=0 (tests): the fused wide kernels exist as 8-wave kernels only
  return x3_fused_mode() == 1 || x3_fused_mode() == 2 || (x3_fused_mode() == 3 && tile != TILE_256x320);
}

// Which 3x3x3 stages of the split-bf16 mode run in their Winograd form (wino.hip).  BSMI_WINO: 0 = none, unset / 1 = where it
// was measured to win on the 128^3 block -- the stages with at least 256 channels on both sides, whose matrix work outweighs
// the transform passes over the layer's tensors (ms direct -> Winograd: 1500 -> 1500 12.19 -> 7.07, 1800 -> 300 10.55 -> 7.63,
// 300 -> 1500 3.37 -> 2.27, 300 -> 300 3.22 -> 2.90 and 2.23 -> 2.03; narrower stages lose: 360 -> 60 2.48 -> 3.44,
// 60 -> 300 0.91 -> 1.20) --, 2 = every stage the kernels can take (tests: small nets).
static int wino_mode() {
  static const int m = [] { const char* e = getenv("BSMI_WINO"); return e ? atoi(e) : 1; }();
  return m;
}

// Which Winograd stages use the F(4x4, 3x3) tile (round 4): 36 products per 16 outputs instead of 16 per 4.  BSMI_WINO4: 0 =
// none (F(2x2) as in round 3), unset / 1 = every Winograd stage, 2 = the same (kept for the tests' spelling).  Measured on the
// 128^3 block (ms F(2x2) -> F(4x4)): 1500 -> 1500 6.99 -> 4.27, 1800 -> 300 7.07 -> 4.67, 300 -> 300 2.90 -> 1.82 and 1.90 ->
// 1.38, 300 -> 1500 2.22 -> 1.50; block 28.3 -> 20.5 ms.  Error of the whole net against the CPU fp32 oracle 8.6e-6 -> 9.0e-6
// (gate 1e-4): the interpolation points 0, +-1/sqrt2, +-sqrt2, inf keep a layer's error at four times F(2x2)'s where the
// textbook points 0, +-1, +-2 make it fifteen times (wino.hip), and a layer's error reaches the sigmoid outputs attenuated.
static int wino4_mode() {
  static const int m = [] { const char* e = getenv("BSMI_WINO4"); return e ? atoi(e) : 1; }();
  return m;
}
int wino_tile_edge() { return wino4_mode() == 0 ? 2 : 4; }

// The last stage of a decoder ConvPass is a special case (wino_narrow_last below): behind a (1,2,2) upsampling it runs in
// Winograd form whenever the pass's first stage does, whatever its own cin * cout, because only then can Planner::rec fuse the
// upsampling into the pass -- and the upsampled map, its launch and three quarters of the first stage's source reads, is what
// the pass spends most on (360 -> 60, 60 -> 60 of the 128^3 block: DESIGN.md section 6).  Such a stage takes the form ONLY
// behind a fused upsampling (PackedWino::fused_only); every other site keeps the thresholds below, the encoder's 60 -> 60
// stage among them.
bool wino_eligible(const PassSite& p, int ci) {
  if (wino_mode() == 0 || p.k[ci][0] != 3 || p.k[ci][1] != 3 || p.k[ci][2] != 3) return false;
  if (ci == 0 && p.nslots > kWinoMaxSrc) return false;
  if (!x3_fused_for(choose_tile(p.cout))) return false;
  if (wino_mode() >= 2) return true;
  int cin = p.cout;
  if (ci == 0) {
    cin = 0;
    for (int s = 0; s < p.nslots; ++s) cin += p.cin[s];
  }
  if (cin >= 256 && p.cout >= 256) return true;
  // with F(4x4) tiles (V 2.25x the input instead of 4x, 2.25 sums per output instead of 4) two narrower stages win as well,
  // measured on the 128^3 block: 60 -> 300 0.88 -> 0.80 ms, 360 -> 60 2.09 -> 1.94 (60 -> 60 0.87 -> 1.23 and the 12-channel
  // stages lose)
  return wino4_mode() == 1 && (int64_t)cin * p.cout >= 16384 && cin >= 32 && p.cout >= 32;
}

// BSMI_FUSE_UP_NARROW=0: a decoder pass fuses its upsampling only when its last stage is a Winograd stage by wino_eligible's own
// thresholds (the rule before this one; kept for A/B runs and as the cross-check).
static bool fuse_up_narrow() {
  static const bool on = [] { const char* e = getenv("BSMI_FUSE_UP_NARROW"); return !(e && e[0] == '0'); }();
  return on;
}
// The narrow last stage of decoder pass `p` that takes the Winograd form for the sake of the fused upsampling.
bool wino_narrow_last(const bsmi_unet* h, const PassSite& p, int ci) {
  if (!fuse_up_narrow() || wino_mode() == 0 || p.nslots != 2 || p.nconv < 2 || ci != p.nconv - 1) return false;
  if (&p < h->r_conv.data() || &p >= h->r_conv.data() + h->r_conv.size()) return false;
  const int* f = h->cfg.downsample_factors[&p - h->r_conv.data()];
  if (f[0] != 1 || f[1] != 2 || f[2] != 2) return false;   // what Planner::rec can fuse
  if (p.k[ci][0] != 3 || p.k[ci][1] != 3 || p.k[ci][2] != 3 || p.cout < 32 || !x3_fused_for(choose_tile(p.cout))) return false;
  return wino_eligible(p, 0) && !wino_eligible(p, ci);
}

// Which first stages of a decoder pass behind a fused (1,2,2) upsampling convolve their upsampled source BELOW the upsampling
// (PackedWino::below_*).  BSMI_CONV_BELOW_UP, read once per process: 0 = none (the F(4x4) form over both
// sources, as before), 1 = every such stage, unset = the rule: every such stage as well, since both stages of the 128^3 block
// that have the form gain by more than the spread of three repeats (ms per launch, tools/probe_unet.py bf16x3: 1800 -> 300
// 4.51-4.55 -> 4.00-4.12, 360 -> 60 1.64 -> 1.05-1.07).  A stage that loses would be excluded here.
static int conv_below_up_mode() {
  static const int m = [] { const char* e = getenv("BSMI_CONV_BELOW_UP"); return e ? atoi(e) : -1; }();
  return m;
}
bool below_up_site(const bsmi_unet* h, const PassSite& p, int ci) {
  if (conv_below_up_mode() == 0 || ci != 0 || p.nslots != 2 || p.nconv < 2 || !wino_eligible(p, 0)) return false;
  if (&p < h->r_conv.data() || &p >= h->r_conv.data() + h->r_conv.size()) return false;
  const int* f = h->cfg.downsample_factors[&p - h->r_conv.data()];
  if (f[0] != 1 || f[1] != 2 || f[2] != 2) return false;   // what Planner::rec can fuse
  if (p.cout <= 64 && !x3_fused_for(TILE_256x320)) return false;
  return true;
}

// BSMI_FUSE_UP=0: no upsampling is fused into the ConvPass behind it (Planner::rec states when one can be, and what it saves).
bool fuse_up_enabled() {
  static const bool on = [] { const char* e = getenv("BSMI_FUSE_UP"); return !(e && e[0] == '0'); }();
  return on;
}
// BSMI_POOL_FUSE=0: no pooling is stored by the output transform of the stage before it (Planner::rec, fused pooling).
bool pool_fuse_enabled() {
  static const bool pool_fuse = [] { const char* e = getenv("BSMI_POOL_FUSE"); return !(e && e[0] == '0'); }();
  return pool_fuse;
}

// Which F(4x4) stages take the "wz" form, F(2,3) along z as well (wino.h WinoInArgs::wz): 144 batches of
// K = Cin over pairs of output planes instead of 36 of K = 3 Cin over planes, two thirds of the multiplies, V and M twice the
// size.  BSMI_WINO_Z, read once per process: 0 = none, 1 = every stage the kernels can take (tests), unset = the rule.
// The kernels take a stage whose transforms carry nothing else: no source read through a fused upsampling and no sums from
// below it (the first and the last stage of a decoder pass behind a (1,2,2) upsampling), no pooled output (the last stage of
// an encoder pass before a (1,2,2) pooling) -- those keep the plain F(4x4) form, decided here from the site alone so that one
// set of weight images is packed.
static int wino_z_mode() {
  static const int m = [] { const char* e = getenv("BSMI_WINO_Z"); return e ? atoi(e) : -1; }();
  return m;
}
bool wino_z_site(const bsmi_unet* h, const PassSite& p, int ci) {
  if (wino_z_mode() == 0 || wino_tile_edge() != 4 || !wino_eligible(p, ci)) return false;
  int cin = p.cout;
  if (ci == 0) {
    cin = 0;
    for (int s = 0; s < p.nslots; ++s) cin += p.cin[s];
  }
  if (&p >= h->r_conv.data() && &p < h->r_conv.data() + h->r_conv.size()) {
    const int* f = h->cfg.downsample_factors[&p - h->r_conv.data()];
    const bool fusable = fuse_up_enabled() && p.nslots == 2 && f[0] == 1 && f[1] == 2 && f[2] == 2;   // what Planner::rec can fuse
    if (fusable && (ci == 0 || ci == p.nconv - 1)) return false;
  } else if (&p >= h->l_conv.data() && &p < h->l_conv.data() + h->l_conv.size()) {
    const size_t i = &p - h->l_conv.data();
    if (i + 1 < h->l_conv.size() && ci == p.nconv - 1) {   // a pooling follows
      const int* f = h->cfg.downsample_factors[i];
      if (pool_fuse_enabled() && f[0] == 1 && f[1] == 2 && f[2] == 2) return false;
    }
  } else {
    return false;
  }
  if (wino_z_mode() >= 1) return true;
  // The rule: the stages measured to gain more than the spread of three repeats of tools/probe_unet.py bf16x3 on the 128^3
  // block (ms per launch, min-max, BSMI_WINO_Z=0 -> 1): 1500 -> 1500 4.09-4.20 -> 3.80-3.88 gains;
  // 300 -> 1500 1.48-1.51 -> 1.73-1.74 and 60 -> 300 0.77-0.78 -> 1.28-1.29 lose.  Both 300 -> 300 stages of that block cannot take
  // the form (one stores the pooled output, the other is the last stage of a fused decoder pass: 1.79-1.81 and 1.22-1.24 either
  // way), nor can 1800 -> 300.  A batch of the wz GEMM gives the matrix pipe 6 R Cin Npad FLOP for 4 R (Cin + Npad) bytes of V and
  // M: 1140 FLOP/B for 1504 -> 1536, 381 and 80 for the two losers against the chip's balance of about 500 -- below it the doubled
  // V and M cost more than the multiplies return.  Hence both sides at least 1024 channels.
  return cin >= 1024 && p.cout >= 1024;
}

// Which stages run in the halo-resident form (conv_h16.hip).  BSMI_H16: 0 = none, unset / 1 = the stages with at most 64 output
// channels whose launch is large enough to fill the chip, 2 = every stage the kernel can take (tests: small nets).
int h16_mode() {
  static const int m = [] { const char* e = getenv("BSMI_H16"); return e ? atoi(e) : 1; }();
  return m;
}
int h16_only_npad() {
  static const int only_npad = [] { const char* e = getenv("BSMI_H16_NPAD"); return e ? atoi(e) : 0; }();  // dev: one column count only
  return only_npad;
}
// BSMI_H16_BALANCE=0: the halo-resident launch is not tiled to the CU count (h16_tiling)
bool h16_balanced() {
  static const bool balanced = [] { const char* e = getenv("BSMI_H16_BALANCE"); return !(e && e[0] == '0'); }();
  return balanced;
}

// Whether a stage of `nsteps` K-steps on `tile` may take the raster-halo form (conv_rh.hip; Planner::plan_rh checks that the halo fits).
bool rh_enabled(int prec, TileCfg tile, size_t nsteps) {
  // BSMI_USE_RH: 1 = wherever the halo fits, 0 = never, unset = only where it was measured to win on the
  // 128^3 block: small-Cout tiles with a long K loop (the 360->60 channel layer: 1.43 -> 1.04 ms); the rows the
  // raster-halo form computes and drops cost the small-plane layers 8-17 %, and short-K layers do not amortise it
  static const int mode = [] { const char* e = getenv("BSMI_USE_RH"); return !e ? 2 : (e[0] == '1' ? 1 : 0); }();
  // split mode: never (a form that listed the K-steps per plane through the bf16 kernel lost to the fused gather kernel on every
  // layer -- 360 -> 60 channels: 3.16 against 2.41 ms -- and was removed in round 3, as was its fused variant; the halo form of the split mode is Planner::plan_h16)
  return prec != BSMI_PREC_BF16X3 && (mode == 1 || (mode == 2 && tile_bn(tile) <= 64 && nsteps >= 200));
}

// BSMI_USE_BOX: 0 = never, unset / 1 = wherever it applies (Planner::plan_box: bf16, 3x3x3, at most 16 output channels).
bool box_enabled() {
  static const bool enabled = [] { const char* e = getenv("BSMI_USE_BOX"); return !(e && e[0] == '0'); }();
  return enabled;
}

// The first ConvPass can run as one launch (first_pass.hip): one raw channel, two 3x3x3 convs, at most 16 feature maps.
bool first_pass_eligible(const bsmi_unet* h) {
  if (h->cfg.in_channels != 1 || h->l_conv.empty()) return false;
  const PassSite& p = h->l_conv[0];
  if (p.nconv != 2 || p.cout > 16) return false;
  for (int c = 0; c < 2; ++c)
    for (int d = 0; d < 3; ++d)
      if (p.k[c][d] != 3) return false;
  const char* e = getenv("BSMI_FUSED_FIRST");
  return !(e && e[0] == '0');
}

}  // namespace bsmi

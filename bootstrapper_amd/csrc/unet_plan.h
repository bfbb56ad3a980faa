// The planner of the U-Net engine, shared by the two files that define it: unet_plan.hip (the walk over the network and the
// direct forms of a stage) and unet_plan_wino.hip (the Winograd form).  Nobody else includes this.
#pragma once
#include "unet_internal.h"

namespace bsmi {

// An upsampled map whose only readers are Winograd stages of the ConvPass that follows it (its first stage's taps, its
// last stage's residual branch): the stages read the LOW-resolution tensor and interpolate on the fly, the UP step is skipped.
struct UpFuse {
  TDesc low;    // the tensor below the upsampling
  int f[3];     // factors (1, f, f)
  int o[3];     // crop offset of the upsampled map inside the full upsampling (Upsample.crop_to_factor, unet.py:177-183)
};

struct Planner {
  bsmi_unet* h;
  int prec;
  Plan* plan;
  bool dry;  // shape / flop arithmetic only: no allocation, no device traffic
  const UpFuse* fuse_up = nullptr;  // set while the ConvPass behind a fused upsampling is planned

  int alloc(TDesc& t);
  int plan_rh(const PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st);
  int plan_h16(PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st);
  int plan_box(const PassSite& p, int ci, const TDesc* slots, const int (*so)[3], const TDesc& o, PlanStep& st);
  int plan_wino(PassSite& p, int ci, const PackedConv& pc, const TDesc* slots, const int (*so)[3], int nsl, const TDesc& o, PlanStep& st);  // unet_plan_wino.hip
  int pass(PassSite& p, const TDesc* in, const int (*org)[3], const int sp_in[3], TDesc& out);
  int rec(int level, const TDesc& f_in, TDesc& f_out);
  int run(const int64_t in_shape[3]);
};

// the K-step table of launch `a`: uploaded, owned by the plan
int upload_ksteps(Plan* plan, const std::vector<KStep>& ks, ConvArgs& a);
// every source slot of `a` = one channels-last tensor at `base`: rows of W voxels, planes of H rows, C channels of `bytes_per_channel`
void set_strides(ConvArgs& a, const void* base, int H, int W, int C, int bytes_per_channel);

}  // namespace bsmi

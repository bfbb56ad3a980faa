// Training engine: the packed weight, bias and head images of the step's launches, rewritten on the device from the flat
// parameter buffer after every optimizer step (train_internal.h has the file map and says which stream packs what).
//   pack_weights_kernel            f32 image of a forward or input-gradient launch
//   pack_weights_x3_kernel         hi / lo images of a fused split-bf16 launch; pack_weights_x3_t_kernel: the same through LDS
//   pack_bias_kernel, pack_head_kernel
// A PackJob is one image and the list of PackUnits it is gathered from; begin makes them (make_forward_job here,
// make_forward_x3 and make_dgrad in train_plan.hip) and run_pack_jobs launches a named subset of them.
#include <cstdlib>

#include "train_internal.h"

namespace bsmi {

__global__ void pack_weights_kernel(const float* __restrict__ params, const PackUnit* __restrict__ units, int nunits, int Npad,
                                    int nreal, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (unit, n)
  if (i >= (size_t)nunits * Npad) return;
  const int u = (int)(i / Npad), n = (int)(i - (size_t)u * Npad);
  const PackUnit pu = units[u];
  float v[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    v[kk] = 0.f;
    if (pu.wbase >= 0 && n < nreal && pu.c0 + kk < pu.creal) v[kk] = params[pu.wbase + (long long)n * pu.sn + (long long)(pu.c0 + kk) * pu.sc + pu.tap];
  }
  float* d = dst + ((size_t)(u >> 1) * Npad + n) * 16 + (u & 1) * 8;
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) d[kk] = v[kk];
}

// the same for a fused split-bf16 launch: units of 16 channels, rows of 32 bf16, a hi image and a lo image (conv_igemm.h)
// Thread -> (unit, n): the units of a window of `ugw` consecutive units (the taps x 2 units of a 32-channel chunk) vary
// fastest, then n: consecutive lanes then read consecutive taps of one (n, c) -- and the next n or c continues the run --
// instead of one cache line per lane (n fastest: 2.9 ms per step for the two images of every layer).
__global__ void pack_weights_x3_kernel(const float* __restrict__ params, const PackUnit* __restrict__ units, int nunits, int Npad, int nreal,
                                       int ugw, uint32_t* __restrict__ hi_img, uint32_t* __restrict__ lo_img) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per_window = (size_t)ugw * Npad;
  const int win = (int)(i / per_window);
  const size_t r = i - (size_t)win * per_window;
  const int n = (int)(r / ugw), u = win * ugw + (int)(r - (size_t)n * ugw);
  if (u >= nunits) return;
  const PackUnit pu = units[u];
  const size_t d = (((size_t)(u >> 1) * Npad + n) * 32 + (u & 1) * 16) / 2;  // in bf16 pairs
#pragma unroll
  for (int kk = 0; kk < 16; kk += 2) {
    float v0 = 0.f, v1 = 0.f;
    if (pu.wbase >= 0 && n < nreal) {
      if (pu.c0 + kk < pu.creal) v0 = params[pu.wbase + (long long)n * pu.sn + (long long)(pu.c0 + kk) * pu.sc + pu.tap];
      if (pu.c0 + kk + 1 < pu.creal) v1 = params[pu.wbase + (long long)n * pu.sn + (long long)(pu.c0 + kk + 1) * pu.sc + pu.tap];
    }
    uint32_t h, l;
    split_pair(v0, v1, h, l);
    hi_img[d + kk / 2] = h;
    lo_img[d + kk / 2] = l;
  }
}

// The same through LDS, for windows of a 3 x 3 x 3 layer (ugw = 2 x 27 units of one 32-channel chunk, ordered [tap][half]): a
// workgroup takes PK_NB output channels of one window, reads their 32 x 27 weights in the order they lie in the parameter
// buffer (one run of 3 456 bytes per output channel; the kernel above has every lane walk its own 16 channels, 108 bytes
// apart) and writes the K-steps' rows PK_NB at a time (512 contiguous bytes per image and K-step instead of 32).  The unit
// fields are used as they are: a window that is not of that form (a residual's, padding) is packed correctly, only slower.
constexpr int PK_NB = 8;
template <int NT>  // taps per window (27: constant divisors); 0: ugw / 2 at run time
__global__ __launch_bounds__(256) void pack_weights_x3_t_kernel(const float* __restrict__ params, const PackUnit* __restrict__ units, int nunits,
                                                                int Npad, int nreal, int ugw, uint32_t* __restrict__ hi_img,
                                                                uint32_t* __restrict__ lo_img) {
  extern __shared__ __attribute__((aligned(16))) float pk_sv[];  // [PK_NB][32 channels][taps] values (the order of an OIDHW weight), then the window's units
  PackUnit* su = (PackUnit*)(pk_sv + (size_t)PK_NB * ugw * 16);
  const int tid = threadIdx.x;
  const int nt = NT ? NT : ugw / 2;
  const int u0 = blockIdx.x * ugw, n0 = blockIdx.y * PK_NB;
  for (int i = tid; i < ugw; i += 256) {  // (straight into LDS: a local copy of the struct was a scratch segment)
    if (u0 + i < nunits) {
      su[i] = units[u0 + i];
    } else {
      su[i] = PackUnit{};
      su[i].wbase = -1;
    }
  }
  __syncthreads();
  const int per_n = 32 * nt;
  // forward image: n is the weight's output channel (the outermost index of OIDHW): tap fastest, then the chunk's 32 channels;
  // input-gradient image: n is the weight's INPUT channel (make_dgrad: sn = taps): tap fastest, then the PK_NB values of n
  const bool n_inner = su[0].wbase >= 0 && su[0].sn < su[0].sc;
  for (int e = tid; e < PK_NB * per_n; e += 256) {
    int nl, c, tap;
    if (n_inner) {
      c = e / (PK_NB * nt);
      const int r = e - c * (PK_NB * nt);
      nl = r / nt;
      tap = r - nl * nt;
    } else {
      nl = e / per_n;
      const int r = e - nl * per_n;
      c = r / nt;
      tap = r - c * nt;
    }
    const PackUnit& pu = su[tap * 2 + (c >> 4)];
    const int n = n0 + nl, kk = c & 15;
    float v = 0.f;
    if (pu.wbase >= 0 && n < nreal && pu.c0 + kk < pu.creal) v = params[pu.wbase + (long long)n * pu.sn + (long long)(pu.c0 + kk) * pu.sc + pu.tap];
    pk_sv[nl * per_n + c * nt + tap] = v;  // consecutive lanes, consecutive words (a [unit][16] layout: one bank for the whole wave)
  }
  __syncthreads();
  for (int e = tid; e < ugw * PK_NB * 8; e += 256) {
    const int pr = e & 7, half = (e >> 3) & 1, nl = (e >> 4) % PK_NB, ksl = e / (16 * PK_NB);
    const int ul = ksl * 2 + half, u = u0 + ul, n = n0 + nl;
    if (u >= nunits || n >= Npad) continue;
    const float* v = pk_sv + nl * per_n + (half * 16 + 2 * pr) * nt + ksl;
    uint32_t h, l;
    split_pair(v[0], v[nt], h, l);
    const size_t d = (((size_t)(u >> 1) * Npad + n) * 32 + (u & 1) * 16) / 2 + pr;
    hi_img[d] = h;
    lo_img[d] = l;
  }
}

// bias image of a forward launch: b[n] = params[b0 + n] (+ params[b1 + n])
__global__ void pack_bias_kernel(const float* __restrict__ params, long long b0, long long b1, int nreal, int Npad, float* __restrict__ dst) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Npad) return;
  float v = 0.f;
  if (n < nreal) v = params[b0 + n] + (b1 >= 0 ? params[b1 + n] : 0.f);
  dst[n] = v;
}

// head image [cout][2][cin] / [cout][2] from the two 1x1x1 weights
__global__ void pack_head_kernel(const float* __restrict__ params, long long wc, long long wr, long long bc, long long br, int cout, int cin,
                                 float* __restrict__ hw, float* __restrict__ hb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cout * cin) {
    const int o = i / cin, c = i - o * cin;
    hw[(o * 2 + 0) * cin + c] = params[wc + i];
    hw[(o * 2 + 1) * cin + c] = params[wr + i];
  }
  if (i < cout) {
    hb[i * 2 + 0] = params[bc + i];
    hb[i * 2 + 1] = params[br + i];
  }
}

int upload_units(TrainState* ts, const std::vector<PackUnit>& u, PackUnit** dev) {
  int rc = talloc(ts, (void**)dev, u.size() * sizeof(PackUnit), false);
  if (rc) return rc;
  BSMI_HIP(hipMemcpy(*dev, u.data(), u.size() * sizeof(PackUnit), hipMemcpyHostToDevice));
  return BSMI_OK;
}

std::vector<PackUnit> entry_units(const std::vector<PackEntry>& ents, const StageParams& par) {
  const std::vector<int64_t>&wm = par.w->shape, &wr = par.rw->shape;  // OIDHW
  const int64_t cin_m = wm[1], ntap = wm[2] * wm[3] * wm[4], cin_r = wr[1];
  std::vector<PackUnit> units(ents.size());
  for (size_t u = 0; u < ents.size(); ++u) {
    const PackEntry& e = ents[u];
    PackUnit pu{};
    if (e.dummy) {
      pu.wbase = -1;
    } else if (e.wsrc == 0) {
      pu.wbase = (long long)par.w->off + (long long)e.cin_base * ntap;
      pu.sn = (int)(cin_m * ntap); pu.sc = (int)ntap; pu.tap = e.tap;
    } else {
      pu.wbase = (long long)par.rw->off + e.cin_base;
      pu.sn = (int)cin_r; pu.sc = 1; pu.tap = 0;
    }
    pu.c0 = e.c0;
    pu.creal = e.creal;
    units[u] = pu;
  }
  return units;
}

// pack job of a forward launch: the unit list is the one the planner packed from (build_entries)
int make_forward_job(TrainState* ts, PassSite& p, int ci) {
  PackedConv& pc = p.packed[BSMI_PREC_F32][ci];
  StageParams par;
  int rc = find_stage_params(ts, p.prefix, ci, &par);
  if (rc) return rc;
  const std::vector<PackUnit> units = entry_units(pc.entries, par);
  PackJob job;
  if ((rc = upload_units(ts, units, &job.units))) return rc;
  job.nunits = (int)units.size();
  job.Npad = pc.Npad;
  job.nreal = p.cout;
  job.dst = (float*)pc.w;
  job.b0 = (long long)par.b->off;
  job.b1 = ci == p.nconv - 1 ? (long long)par.rb->off : -1;
  job.bias_dst = pc.bias;
  ts->fwd_job_of[pc.bias] = ts->jobs.size();
  ts->jobs.push_back(job);
  return BSMI_OK;
}

static void pack_f32_image(const TrainState* ts, const PackJob& j, hipStream_t s) {
  hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)(((size_t)j.nunits * j.Npad + 255) / 256)), dim3(256), 0, s, (const float*)ts->w,
                     (const PackUnit*)j.units, j.nunits, j.Npad, j.nreal, j.dst);
}

static void pack_x3_images(const TrainState* ts, const PackJob& j, hipStream_t s) {
  const int ugw = std::max(2, j.window);
  static const bool pack_t = env_on("BSMI_PACK_T");
  if (ugw >= 16 && ugw % 2 == 0 && j.Npad % PK_NB == 0 && pack_t) {
    const size_t lds = (size_t)PK_NB * ugw * 16 * sizeof(float) + (size_t)ugw * sizeof(PackUnit);
    const dim3 grid((unsigned)((j.nunits + ugw - 1) / ugw), (unsigned)(j.Npad / PK_NB));
    hipLaunchKernelGGL(ugw == 54 ? pack_weights_x3_t_kernel<27> : pack_weights_x3_t_kernel<0>, grid, dim3(256), lds, s, (const float*)ts->w,
                       (const PackUnit*)j.units, j.nunits, j.Npad, j.nreal, ugw, j.dst_hi, j.dst_lo);
  } else {
    const size_t padded = (size_t)((j.nunits + ugw - 1) / ugw) * ugw * j.Npad;
    hipLaunchKernelGGL(pack_weights_x3_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, s, (const float*)ts->w,
                       (const PackUnit*)j.units, j.nunits, j.Npad, j.nreal, ugw, j.dst_hi, j.dst_lo);
  }
}

int run_pack_jobs(TrainState* ts, hipStream_t s, PackSet set, PackF32 f32) {
  for (const PackJob& j : ts->jobs) {
    if (set == PACK_FWD_EARLY && (j.backward || j.late)) continue;
    if (set == PACK_BWD && !j.backward) continue;
    if (set == PACK_FWD_LATE && !j.late) continue;
    if (j.dst_hi)
      pack_x3_images(ts, j, s);
    else if (!(f32 == F32_LAZY && j.shadowed))
      pack_f32_image(ts, j, s);
    if (j.bias_dst)
      hipLaunchKernelGGL(pack_bias_kernel, dim3((j.Npad + 255) / 256), dim3(256), 0, s, (const float*)ts->w, j.b0, j.b1, j.nreal, j.Npad, j.bias_dst);
  }
  if (f32 == F32_LAZY) ts->f32_images_stale = true;
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

// the f32 weight images that F32_LAZY packs have left behind the parameters (their bias images are current)
int train_refresh_f32_images(bsmi_unet* h, hipStream_t s) {
  TrainState* ts = h->train;
  if (!ts || !ts->f32_images_stale) return BSMI_OK;
  for (const PackJob& j : ts->jobs)
    if (j.shadowed) pack_f32_image(ts, j, s);
  ts->f32_images_stale = false;
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

void launch_pack_head(const TrainState* ts, const HeadSite& hd, const StageParams& par, hipStream_t s) {
  hipLaunchKernelGGL(pack_head_kernel, dim3((hd.cout * hd.cin + 255) / 256), dim3(256), 0, s, (const float*)ts->w, (long long)par.w->off,
                     (long long)par.rw->off, (long long)par.b->off, (long long)par.rb->off, hd.cout, hd.cin, hd.hw, hd.hb);
}

}  // namespace bsmi

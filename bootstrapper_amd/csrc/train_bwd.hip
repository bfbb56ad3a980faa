// Training engine: the element-wise and reduction kernels of the step and one launcher per plan-step type.  Everything here
// runs on the caller's stream (train_internal.h has the file map and the stream rules).
//   loss       loss_sums_kernel -> [fold_kernel] -> loss_grad_kernel                       launch_loss
//   HEAD       head_bwd_kernel [-> fold_kernel x 2]                                        launch_head_bwd
//   UP         upsample_bwd_kernel | upsample_bwd_gather_kernel (deterministic mode)      launch_up_bwd
//   POOL       maxpool_bwd_kernel                                                          launch_pool_bwd
//   CONV       relu_bwd_pad_kernel [-> colsum_kernel [-> fold_kernel]]                     launch_mask_pad_bias
//              scatter_add_kernel per source of a pass's first stage                       launch_scatter
//   f32_to_split_kernel, split_to_f32_kernel: around the fused split-bf16 launches of the forward pass (train_plan.hip) and
//   of the input gradient (train.hip)                                                      launch_f32_to_split, launch_split_to_f32
//   adam_kernel                                                                            launch_adam
// Deterministic mode (bsmi_unet_train_set_deterministic) replaces every float atomic by per-workgroup partial sums in
// TrainState::det_part / loss_part that fold_kernel adds in index order.
#include <cmath>
#include <cstdlib>
#include <numeric>

#include "train_internal.h"

namespace bsmi {

// WeightedMSELoss, pass 1: sums[0] += sum of w (p - t)^2 over w > 0, sums[1] += count(w > 0), sums[2] += sum over all,
// sums[3] += count(scale != 0)
// `part` (deterministic mode): instead of the atomics every workgroup leaves its four sums in part[block][4] (its waves folded
// in wave order) and fold_kernel adds the workgroups in index order.
__global__ void loss_sums_kernel(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ w, size_t n,
                                 double* __restrict__ sums, double* __restrict__ part) {
  __shared__ double wave_sums[16][4];
  double s_mask = 0, s_all = 0;
  unsigned long long c_mask = 0, c_nz = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = p[i] - t[i];
    const float sc = w[i] * (d * d);
    s_all += sc;
    if (w[i] > 0.f) { s_mask += sc; ++c_mask; }
    if (sc != 0.f) ++c_nz;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s_mask += __shfl_down(s_mask, o);
    s_all += __shfl_down(s_all, o);
    c_mask += __shfl_down(c_mask, o);
    c_nz += __shfl_down(c_nz, o);
  }
  if (part) {
    if ((threadIdx.x & 63) == 0) {
      double* ws = wave_sums[threadIdx.x >> 6];
      ws[0] = s_mask; ws[1] = (double)c_mask; ws[2] = s_all; ws[3] = (double)c_nz;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      double acc = 0;
      for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) acc += wave_sums[wv][threadIdx.x];
      part[(size_t)blockIdx.x * 4 + threadIdx.x] = acc;
    }
    return;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&sums[0], s_mask);
    atomicAdd(&sums[1], (double)c_mask);
    atomicAdd(&sums[2], s_all);
    atomicAdd(&sums[3], (double)c_nz);
  }
}

// Ordered fold of per-workgroup partial sums (deterministic mode): out[i] (+)= part[0][i] + part[1][i] + ... in that order, one
// thread per column i < width; rows are `stride` values apart.  The same bits whatever order the workgroups ran in.
template <typename T>
__global__ __launch_bounds__(1024) void fold_kernel(const T* __restrict__ part, int nparts, int stride, int width, T* __restrict__ out0,
                                                    T* __restrict__ out1, int assign) {
  // a workgroup = 32 columns x 32 chunk lanes: lane l adds rows l, l + 32, l + 64, ... in that order, then the 32 lanes' sums are
  // added in lane order -- a fixed tree, whatever the order the partial results were produced in
  __shared__ T lanes[32][33];
  const int col = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + col;
  T acc = 0;
  if (i < width) {
    int pidx = l;
    for (; pidx + 96 < nparts; pidx += 128) {  // four loads in flight, added in row order
      const T a0 = part[(size_t)pidx * stride + i], a1 = part[(size_t)(pidx + 32) * stride + i];
      const T a2 = part[(size_t)(pidx + 64) * stride + i], a3 = part[(size_t)(pidx + 96) * stride + i];
      acc += a0; acc += a1; acc += a2; acc += a3;
    }
    for (; pidx < nparts; pidx += 32) acc += part[(size_t)pidx * stride + i];
  }
  lanes[l][col] = acc;
  __syncthreads();
  if (l != 0 || i >= width) return;
  T sum = 0;
  for (int k = 0; k < 32; ++k) sum += lanes[k][col];
  if (assign) {
    out0[i] = sum;
    if (out1) out1[i] = sum;
  } else {
    out0[i] += sum;
    if (out1) out1[i] += sum;
  }
}

// pass 2: loss value and dL/dp; dp = 2 w (p - t) / N with N = count(w > 0) if any weighted error is non-zero, else numel
__global__ void loss_grad_kernel(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ w, size_t n,
                                 const double* __restrict__ sums, float* __restrict__ dp, float* __restrict__ loss_accum) {
  const bool masked = sums[3] != 0.0;
  const double denom = masked ? sums[1] : (double)n;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(loss_accum, (float)((masked ? sums[0] : sums[2]) / denom));
  const float inv = (float)(1.0 / denom);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float g = 2.f * w[i] * (p[i] - t[i]) * inv;
    dp[i] = (masked && !(w[i] > 0.f)) ? 0.f : g;
  }
}

// head backward: p = sigmoid((Wc + Wr) z + bc + br).  dlogit = dp p (1 - p); dz (channels-last) += (Wc + Wr)^T dlogit;
// dWc, dWr += dlogit z^T; dbc, dbr += dlogit.  One thread per voxel, block-level reduction of the weight gradients.
// WIDE: more than 32 input channels (up to the 64 of the forward's head kernel): the voxel's channels are read where they are
// used instead of being kept in a private array; the sums and their order are the same.
template <bool WIDE>
__global__ void head_bwd_kernel(const float* __restrict__ z, int zc, const float* __restrict__ p, const float* __restrict__ dp, size_t nvox,
                                int cin, int cout, const float* __restrict__ hw, float* __restrict__ dz, float* __restrict__ gwc,
                                float* __restrict__ gwr, float* __restrict__ gbc, float* __restrict__ gbr, float* __restrict__ part) {
  extern __shared__ float red[];  // [cout * cin + cout]; deterministic mode: one such row per wave
  const int nred = cout * cin + cout;
  for (int i = threadIdx.x; i < nred; i += blockDim.x) red[i] = 0.f;
  __syncthreads();
  const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (part) {
    // deterministic mode: every product is summed over the wave by a fixed shuffle tree (lanes past the end hold zeros), the
    // waves in wave order, and the workgroup's row goes to part[block][nred] for fold_kernel: no atomics anywhere
    const bool live = v < nvox;
    const size_t vv = live ? v : 0;
    float* mine = red + (threadIdx.x >> 6) * nred;
    for (int c = 0; c < cin; ++c) {
      float acc = 0.f;
      for (int o = 0; o < cout; ++o) {
        const float pp = p[(size_t)o * nvox + vv];
        acc += (hw[(o * 2 + 0) * cin + c] + hw[(o * 2 + 1) * cin + c]) * (dp[(size_t)o * nvox + vv] * pp * (1.f - pp));
      }
      if (live) dz[v * zc + c] += acc;
    }
    for (int o = 0; o < cout; ++o) {
      const float pp = p[(size_t)o * nvox + vv];
      const float dlo = live ? dp[(size_t)o * nvox + vv] * pp * (1.f - pp) : 0.f;
      for (int c = 0; c <= cin; ++c) {  // c == cin: the bias column
        float t = c < cin ? dlo * z[vv * zc + c] : dlo;
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
        if ((threadIdx.x & 63) == 0) mine[c < cin ? o * cin + c : cout * cin + o] = t;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nred; i += blockDim.x) {
      float acc = 0.f;
      for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) acc += red[wv * nred + i];
      part[(size_t)blockIdx.x * nred + i] = acc;
    }
    return;
  }
  if (v < nvox) {
    float zz[WIDE ? 1 : 32], dl[16];
    if constexpr (!WIDE)
      for (int c = 0; c < cin; ++c) zz[c] = z[v * zc + c];
    for (int o = 0; o < cout; ++o) {
      const float pp = p[(size_t)o * nvox + v];
      dl[o] = dp[(size_t)o * nvox + v] * pp * (1.f - pp);
    }
    for (int c = 0; c < cin; ++c) {
      float acc = 0.f;
      for (int o = 0; o < cout; ++o) acc += (hw[(o * 2 + 0) * cin + c] + hw[(o * 2 + 1) * cin + c]) * dl[o];
      dz[v * zc + c] += acc;
    }
    for (int o = 0; o < cout; ++o) {
      for (int c = 0; c < cin; ++c) atomicAdd(&red[o * cin + c], dl[o] * (WIDE ? z[v * zc + c] : zz[c]));
      atomicAdd(&red[cout * cin + o], dl[o]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cout * cin; i += blockDim.x) {
    atomicAdd(&gwc[i], red[i]);
    atomicAdd(&gwr[i], red[i]);
  }
  for (int i = threadIdx.x; i < cout; i += blockDim.x) {
    atomicAdd(&gbc[i], red[cout * cin + i]);
    atomicAdd(&gbr[i], red[cout * cin + i]);
  }
}

// g = dY * [Y > 0], written into the interior of a zero-bordered tensor [D + 2pz][H + 2py][W + 2px][C]
// `outs` (optional): the same tensor once more in the split-bf16 activation layout (conv_dev.h act_index: per 8 channels 16
// bytes of hi = bf16(v) then 16 bytes of lo = bf16(v - hi)), the A operand of the split-bf16 input-gradient launch
// `cs0` (optional): the column sums of g -- the bias gradient -- are added to cs0[c] (and cs1[c]) for c < nreal: per workgroup
// in LDS (dynamic, C floats), one global atomic per channel and workgroup at the end (colsum_kernel read the tensor again).
__global__ void relu_bwd_pad_kernel(const float* __restrict__ dy, const float* __restrict__ y, int D, int H, int W, int C, int pz, int py,
                                    int px, float* __restrict__ out, uint16_t* __restrict__ outs, int nreal, float* __restrict__ cs0,
                                    float* __restrict__ cs1) {
  extern __shared__ float rb_sum[];  // [C] when cs0
  if (cs0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) rb_sum[c] = 0.f;
    __syncthreads();
  }
  const size_t total = (size_t)D * H * W * (C / 4);
  const int Hp = H + 2 * py, Wp = W + 2 * px;
  // the channel group of a thread is fixed when the grid's stride is a multiple of C / 4 (the launcher sees to it): sums in registers
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool fixed_c = ((size_t)gridDim.x * blockDim.x) % (size_t)(C / 4) == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % (C / 4));
    size_t v = i / (C / 4);
    const int x = (int)(v % W); v /= W;
    const int yy = (int)(v % H);
    const int zz = (int)(v / H);
    const size_t src = (((size_t)zz * H + yy) * W + x) * C + c4 * 4;
    const float4 g = *(const float4*)(dy + src), a = *(const float4*)(y + src);
    float4 r;
    r.x = a.x > 0.f ? g.x : 0.f; r.y = a.y > 0.f ? g.y : 0.f; r.z = a.z > 0.f ? g.z : 0.f; r.w = a.w > 0.f ? g.w : 0.f;
    const size_t row = (((size_t)(zz + pz) * Hp + (yy + py)) * Wp + (x + px)) * C;
    *(float4*)(out + row + c4 * 4) = r;
    if (cs0) {
      if (fixed_c) {
        acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += r.w;
      } else {
        atomicAdd(&rb_sum[c4 * 4 + 0], r.x); atomicAdd(&rb_sum[c4 * 4 + 1], r.y);
        atomicAdd(&rb_sum[c4 * 4 + 2], r.z); atomicAdd(&rb_sum[c4 * 4 + 3], r.w);
      }
    }
    if (outs) {
      const int n = c4 * 4;
      uint32_t h0, l0, h1, l1;
      split_pair(r.x, r.y, h0, l0);
      split_pair(r.z, r.w, h1, l1);
      uint16_t* d = outs + 2 * row + ((n >> 3) << 4) + (n & 7);
      *(uint2*)d = make_uint2(h0, h1);
      *(uint2*)(d + 8) = make_uint2(l0, l1);
    }
  }
  if (cs0) {
    if (fixed_c) {
      const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
      if (i0 < total) {
        const int c4 = (int)(i0 % (C / 4));
        atomicAdd(&rb_sum[c4 * 4 + 0], acc.x); atomicAdd(&rb_sum[c4 * 4 + 1], acc.y);
        atomicAdd(&rb_sum[c4 * 4 + 2], acc.z); atomicAdd(&rb_sum[c4 * 4 + 3], acc.w);
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C && c < nreal; c += blockDim.x) {
      const float v = rb_sum[c];
      if (v != 0.f) {
        atomicAdd(&cs0[c], v);
        if (cs1) atomicAdd(&cs1[c], v);
      }
    }
  }
}

// split-bf16 copy of an f32 tensor (groups of 8 channels: 16 bytes of hi, 16 bytes of lo)
__global__ void f32_to_split_kernel(const float4* __restrict__ src, uint4* __restrict__ dst, size_t ngroups8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups8; i += (size_t)gridDim.x * blockDim.x) {
    const float4 a = src[2 * i], b = src[2 * i + 1];
    uint4 h, l;
    split_pair(a.x, a.y, h.x, l.x);
    split_pair(a.z, a.w, h.y, l.y);
    split_pair(b.x, b.y, h.z, l.z);
    split_pair(b.z, b.w, h.w, l.w);
    dst[2 * i] = h;
    dst[2 * i + 1] = l;
  }
}

// f32 tensor out of a split-bf16 one (the split-bf16 input-gradient launch writes its result in the activation layout)
__global__ void split_to_f32_kernel(const uint4* __restrict__ src, float4* __restrict__ dst, size_t ngroups8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups8; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 h = src[2 * i], l = src[2 * i + 1];
    float4 a, b;
    a.x = __uint_as_float(h.x << 16) + __uint_as_float(l.x << 16);
    a.y = __uint_as_float(h.x & 0xffff0000u) + __uint_as_float(l.x & 0xffff0000u);
    a.z = __uint_as_float(h.y << 16) + __uint_as_float(l.y << 16);
    a.w = __uint_as_float(h.y & 0xffff0000u) + __uint_as_float(l.y & 0xffff0000u);
    b.x = __uint_as_float(h.z << 16) + __uint_as_float(l.z << 16);
    b.y = __uint_as_float(h.z & 0xffff0000u) + __uint_as_float(l.z & 0xffff0000u);
    b.z = __uint_as_float(h.w << 16) + __uint_as_float(l.w << 16);
    b.w = __uint_as_float(h.w & 0xffff0000u) + __uint_as_float(l.w & 0xffff0000u);
    dst[2 * i] = a;
    dst[2 * i + 1] = b;
  }
}

// column sums of the interior of a padded tensor: out[c0 + c] += sum over voxels of g[..][c0 + c], c < Cc (Cc <= 1024)
__global__ void colsum_kernel(const float* __restrict__ g, int D, int H, int W, int C, int c0, int Cc, int pz, int py, int px, int nreal,
                              float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ part) {
  const int Hp = H + 2 * py, Wp = W + 2 * px;
  const int lanes = blockDim.x / Cc;  // voxels handled side by side
  if ((int)threadIdx.x >= lanes * Cc) return;  // (none: the launcher's block size is a multiple of Cc)
  const int c = c0 + (int)threadIdx.x % Cc;
  // one line of the interior per lane group and trip: no division per element (64-bit ones cost more than the load)
  const int nrows = D * H;
  float acc = 0.f;
  for (int row = (int)blockIdx.x * lanes + (int)threadIdx.x / Cc; row < nrows; row += (int)gridDim.x * lanes) {
    const int zz = row / H, yy = row - zz * H;
    const float* gl = g + (((size_t)(zz + pz) * Hp + (yy + py)) * Wp + px) * C + c;
    float a0 = 0.f, a1 = 0.f;
    int x = 0;
    for (; x + 1 < W; x += 2) {
      a0 += gl[(size_t)x * C];
      a1 += gl[(size_t)(x + 1) * C];
    }
    if (x < W) a0 += gl[(size_t)x * C];
    acc += a0 + a1;
  }
  if (part) {  // deterministic mode: the lane groups in index order, then part[block][C] for fold_kernel
    extern __shared__ float cs_red[];  // [lanes][Cc]
    cs_red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < Cc) {
      float sum = 0.f;
      for (int lg = 0; lg < lanes; ++lg) sum += cs_red[lg * Cc + threadIdx.x];
      part[(size_t)blockIdx.x * C + c] = sum;
    }
    return;
  }
  if (c < nreal && acc != 0.f) {
    atomicAdd(&out0[c], acc);
    if (out1) atomicAdd(&out1[c], acc);
  }
}

// dst[region at (oz, oy, ox)][cdst + c] += src[..][csrc + c] for c < C (gradient of crop + concat)
__global__ void scatter_add_kernel(const float* __restrict__ src, int D, int H, int W, int Cs, int csrc, float* __restrict__ dst, int Hd, int Wd,
                                   int Cd, int cdst, int oz, int oy, int ox, int C) {
  const size_t total = (size_t)D * H * W * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t v = i / C;
    const int x = (int)(v % W); v /= W;
    const int y = (int)(v % H);
    const int z = (int)(v / H);
    dst[(((size_t)(z + oz) * Hd + (y + oy)) * Wd + (x + ox)) * Cd + cdst + c] += src[(((size_t)z * H + y) * W + x) * Cs + csrc + c];
  }
}

// max-pool backward: the gradient of a window goes to its first maximum (torch: strict > while scanning z, y, x)
__global__ void maxpool_bwd_kernel(const float* __restrict__ in, const float* __restrict__ dout, float* __restrict__ din, int H, int W, int C,
                                   int Do, int Ho, int Wo, int fz, int fy, int fx) {
  const size_t total = (size_t)Do * Ho * Wo * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t v = i / C;
    const int x = (int)(v % Wo); v /= Wo;
    const int y = (int)(v % Ho);
    const int z = (int)(v / Ho);
    float best = -INFINITY;
    size_t arg = 0;
    for (int dz = 0; dz < fz; ++dz)
      for (int dy = 0; dy < fy; ++dy)
        for (int dx = 0; dx < fx; ++dx) {
          const size_t s = ((size_t)((z * fz + dz) * H + (y * fy + dy)) * W + (x * fx + dx)) * C + c;
          const float val = in[s];
          if (val > best || (dz == 0 && dy == 0 && dx == 0)) { best = val; arg = s; }
        }
    din[arg] += dout[i];
  }
}

// trilinear upsample (align_corners = False, integer factors) + crop, backward: every output voxel adds its gradient to
// the up-to-8 input voxels it interpolated from (float atomics: windows of neighbouring outputs overlap)
__global__ void upsample_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din, int Di, int Hi, int Wi, int C, int Do, int Ho, int Wo,
                                    int fz, int fy, int fx, int oz, int oy, int ox) {
  const size_t total = (size_t)Do * Ho * Wo * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t v = i / C;
    const int x = (int)(v % Wo) + ox; v /= Wo;
    const int y = (int)(v % Ho) + oy;
    const int z = (int)(v / Ho) + oz;
    const float g = dout[i];
    if (g == 0.f) continue;
    int i0[3], i1[3];
    float w1[3];
    const int pos[3] = {z, y, x}, f[3] = {fz, fy, fx}, n[3] = {Di, Hi, Wi};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float s = ((float)pos[d] + 0.5f) / (float)f[d] - 0.5f;  // torch area_pixel_compute_source_index, align_corners = False
      s = s < 0.f ? 0.f : s;
      i0[d] = (int)s;
      i1[d] = i0[d] + (i0[d] < n[d] - 1 ? 1 : 0);
      w1[d] = s - (float)i0[d];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int iz = (k & 4) ? i1[0] : i0[0], iy = (k & 2) ? i1[1] : i0[1], ix = (k & 1) ? i1[2] : i0[2];
      const float wt = ((k & 4) ? w1[0] : 1.f - w1[0]) * ((k & 2) ? w1[1] : 1.f - w1[1]) * ((k & 1) ? w1[2] : 1.f - w1[2]);
      if (wt != 0.f) atomicAdd(&din[(((size_t)iz * Hi + iy) * Wi + ix) * C + c], g * wt);
    }
  }
}

// The same as a gather (deterministic mode): one thread per INPUT voxel and channel walks the outputs that interpolated from it, in
// z, y, x order, and adds their shares in that order -- no atomics.  Along one axis input j is the lower neighbour (i0) of the
// outputs whose source coordinate lies in [j, j + 1) and the upper one (i1) of those in [j - 1, j): 2 f candidates.
__global__ void upsample_bwd_gather_kernel(const float* __restrict__ dout, float* __restrict__ din, int Di, int Hi, int Wi, int C, int Do, int Ho,
                                           int Wo, int fz, int fy, int fx, int oz, int oy, int ox) {
  const size_t total = (size_t)Di * Hi * Wi * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t v = i / C;
    const int jx = (int)(v % Wi); v /= Wi;
    const int jy = (int)(v % Hi);
    const int jz = (int)(v / Hi);
    // share of output position p (upsampled coordinate) that input j gets along one axis: (1 - w1) if i0 == j, + w1 if i1 == j
    auto share = [](int p, int f, int n, int j, float& lo, float& hi) {
      float s = ((float)p + 0.5f) / (float)f - 0.5f;
      s = s < 0.f ? 0.f : s;
      const int i0 = (int)s, i1 = i0 + (i0 < n - 1 ? 1 : 0);
      const float w1 = s - (float)i0;
      lo = i0 == j ? 1.f - w1 : 0.f;
      hi = i1 == j ? w1 : 0.f;
    };
    float acc = 0.f;
    const int pz0 = max(oz, jz * fz - fz), pz1 = min(oz + Do, jz * fz + 2 * fz);
    const int py0 = max(oy, jy * fy - fy), py1 = min(oy + Ho, jy * fy + 2 * fy);
    const int px0 = max(ox, jx * fx - fx), px1 = min(ox + Wo, jx * fx + 2 * fx);
    for (int pz = pz0; pz < pz1; ++pz) {
      float zl, zh;
      share(pz, fz, Di, jz, zl, zh);
      if (zl == 0.f && zh == 0.f) continue;
      for (int py = py0; py < py1; ++py) {
        float yl, yh;
        share(py, fy, Hi, jy, yl, yh);
        if (yl == 0.f && yh == 0.f) continue;
        for (int px = px0; px < px1; ++px) {
          float xl, xh;
          share(px, fx, Wi, jx, xl, xh);
          if (xl == 0.f && xh == 0.f) continue;
          const float g = dout[(((size_t)(pz - oz) * Ho + (py - oy)) * Wo + (px - ox)) * C + c];
          if (g == 0.f) continue;
          // the eight products of the scatter form, in its order (k = 0 .. 7: z bit 4, y bit 2, x bit 1), those that land on j
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float wt = ((k & 4) ? zh : zl) * ((k & 2) ? yh : yl) * ((k & 1) ? xh : xl);
            if (wt != 0.f) acc += g * wt;
          }
        }
      }
    }
    if (acc != 0.f) din[i] += acc;
  }
}

// torch.optim.Adam (no weight decay, no amsgrad) on flat buffers; gscale folds the 1 / world_size of a summed all-reduce
__global__ void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                            float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float gscale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    // the moments in double, rounded once: in f32 the two terms of m each carry their own roundings, and where the new gradient
    // opposes the old moment the sum is small beside them, so no f32 form keeps m within a few units of ITS OWN last place
    // (tests/test_backward_cpu.py); the kernel is bound by its 28 bytes per element, not by these six operations
    const double gi = (double)g[i] * (double)gscale;
    const float mi = (float)((double)beta1 * (double)m[i] + (1.0 - (double)beta1) * gi);
    const float vi = (float)((double)beta2 * (double)v[i] + (1.0 - (double)beta2) * gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    w[i] = w[i] - (lr / bc1) * (mi / denom);
  }
}

// ------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------
void launch_f32_to_split(const void* src_f32, void* dst_split, size_t ngroups8, hipStream_t s) {
  hipLaunchKernelGGL(f32_to_split_kernel, dim3(grid_1d(ngroups8, 16384)), dim3(256), 0, s, (const float4*)src_f32, (uint4*)dst_split, ngroups8);
}

void launch_split_to_f32(const void* src_split, void* dst_f32, size_t ngroups8, hipStream_t s) {
  hipLaunchKernelGGL(split_to_f32_kernel, dim3(grid_1d(ngroups8, 16384)), dim3(256), 0, s, (const uint4*)src_split, (float4*)dst_f32, ngroups8);
}

// loss of one head added to loss_dev, dL/dp into head_dp
int launch_loss(TrainState* ts, int head, size_t n, const float* target, const float* weight, bool det, hipStream_t s) {
  const float* p = ts->head_out[head];
  BSMI_HIP(hipMemsetAsync(ts->loss_sums, 0, 4 * sizeof(double), s));
  hipLaunchKernelGGL(loss_sums_kernel, dim3(512), dim3(256), 0, s, p, target, weight, n, ts->loss_sums, det ? ts->loss_part : (double*)nullptr);
  if (det) hipLaunchKernelGGL(fold_kernel<double>, dim3(1), dim3(1024), 0, s, (const double*)ts->loss_part, 512, 4, 4, ts->loss_sums, (double*)nullptr, 1);
  hipLaunchKernelGGL(loss_grad_kernel, dim3(512), dim3(256), 0, s, p, target, weight, n, (const double*)ts->loss_sums, ts->head_dp[head], ts->loss_dev);
  return BSMI_OK;
}

// gradients of a head's four parameters and of its input; the head's gradient group is final after it
int launch_head_bwd(bsmi_unet* h, const PlanStep& st, bool det, hipStream_t s) {
  TrainState* ts = h->train;
  const HeadSite& hd = h->heads[st.head];
  const StageParams& par = ts->head_par[st.head];
  TDesc dz = ts->grad_of[st.in.ptr];
  float *gwc = ts->g + par.w->off, *gwr = ts->g + par.rw->off, *gbc = ts->g + par.b->off, *gbr = ts->g + par.rb->off;
  if (hd.cin > 64 || hd.cout > 16) BSMI_FAIL(BSMI_ERR_INVALID, "head backward: at most 64 input and 16 output channels");
  const size_t nv = ts->out_vox;
  const int nred = hd.cout * hd.cin + hd.cout;
  const unsigned hblocks = (unsigned)((nv + 255) / 256);
  int rc;
  if (det && (rc = grow_buf(s, &ts->det_part, &ts->det_part_bytes, (size_t)hblocks * nred * sizeof(float), false))) return rc;
  hipLaunchKernelGGL(hd.cin > 32 ? head_bwd_kernel<true> : head_bwd_kernel<false>, dim3(hblocks), dim3(256), (size_t)(det ? 4 : 1) * nred * sizeof(float), s,
                     (const float*)st.in.ptr, st.in.Cpad, (const float*)ts->head_out[st.head], (const float*)ts->head_dp[st.head], nv, hd.cin,
                     hd.cout, (const float*)hd.hw, (float*)dz.ptr, gwc, gwr, gbc, gbr, det ? (float*)ts->det_part : (float*)nullptr);
  if (det) {  // the workgroups' rows in index order: weights, then biases
    const int nw = hd.cout * hd.cin;
    hipLaunchKernelGGL(fold_kernel<float>, dim3((nw + 31) / 32), dim3(1024), 0, s, (const float*)ts->det_part, (int)hblocks, nred, nw, gwc, gwr, 0);
    hipLaunchKernelGGL(fold_kernel<float>, dim3((hd.cout + 31) / 32), dim3(1024), 0, s, (const float*)ts->det_part + nw, (int)hblocks, nred, hd.cout, gbc, gbr, 0);
  }
  BSMI_HIP(hipEventRecord(ts->groups[ts->group_of[hd.prefix]].ev, s));
  return BSMI_OK;
}

void launch_up_bwd(TrainState* ts, size_t step, bool det, hipStream_t s) {
  const PlanStep& st = ts->plan->steps[step];
  TDesc din = ts->grad_of[st.in.ptr], dout = ts->grad_of[st.out.ptr];
  ts->rec[step].up = det ? 2 : 1;
  // the scatter form has a thread per output element, the gather form (deterministic mode) one per input element
  const TDesc& over = det ? st.in : st.out;
  const size_t total = (size_t)over.D * over.H * over.W * over.Cpad;
  hipLaunchKernelGGL(det ? upsample_bwd_gather_kernel : upsample_bwd_kernel, dim3(grid_1d(total, det ? 65536 : 16384)), dim3(256), 0, s,
                     (const float*)dout.ptr, (float*)din.ptr, st.in.D, st.in.H, st.in.W, st.in.Cpad, st.out.D, st.out.H, st.out.W, st.f[0], st.f[1],
                     st.f[2], st.o[0], st.o[1], st.o[2]);
}

void launch_pool_bwd(TrainState* ts, const PlanStep& st, hipStream_t s) {
  TDesc din = ts->grad_of[st.in.ptr], dout = ts->grad_of[st.out.ptr];
  const size_t total = (size_t)st.out.D * st.out.H * st.out.W * st.out.Cpad;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_1d(total, 16384)), dim3(256), 0, s, (const float*)st.in.ptr, (const float*)dout.ptr,
                     (float*)din.ptr, st.in.H, st.in.W, st.in.Cpad, st.out.D, st.out.H, st.out.W, st.f[0], st.f[1], st.f[2]);
}

int launch_mask_pad_bias(TrainState* ts, size_t step, bool det, hipStream_t s) {
  ConvBwd& cb = ts->convs[step];
  const PlanStep& st = *cb.st;
  const PassSite& p = *st.site;
  TDesc gy = ts->grad_of[st.out.ptr];
  const size_t total4 = (size_t)st.out.D * st.out.H * st.out.W * (st.out.Cpad / 4);
  float* gb = ts->g + cb.par.b->off;
  float* gbr = st.ci == p.nconv - 1 ? ts->g + cb.par.rb->off : nullptr;
  static const bool fuse_colsum = env_on("BSMI_TRAIN_FUSE_COLSUM");
  bsmi_unet_train_step_info& ri = ts->rec[step];
  for (int d = 0; d < 3; ++d) ri.border[d] = cb.P[d];
  ri.has_split = cb.gps ? 1 : 0;
  // fused: the bias gradient (column sums of g) in the same pass: a grid whose stride is a multiple of the channel groups keeps a
  // thread on its four channels; few workgroups, each ends with one atomic per channel
  const bool fused = fuse_colsum && !det;
  ri.bias = fused ? 1 : 2;
  unsigned blocks = grid_1d(total4, fused ? 1024 : 16384);
  const unsigned c4n = st.out.Cpad / 4, q = c4n / std::gcd(c4n, 256u);  // stride = blocks * 256 = 0 mod c4n  <=  blocks = 0 mod (c4n / gcd(c4n, 256))
  if (fused && c4n % 256 != 0 && blocks >= q) blocks = blocks / q * q;
  hipLaunchKernelGGL(relu_bwd_pad_kernel, dim3(blocks), dim3(256), fused ? (size_t)st.out.Cpad * sizeof(float) : 0, s, (const float*)gy.ptr,
                     (const float*)st.out.ptr, st.out.D, st.out.H, st.out.W, st.out.Cpad, cb.P[0], cb.P[1], cb.P[2], (float*)cb.gp.ptr,
                     (uint16_t*)cb.gps, fused ? p.cout : 0, fused ? gb : nullptr, fused ? gbr : nullptr);
  if (fused) return BSMI_OK;
  for (int c0 = 0; c0 < st.out.Cpad; c0 += 512) {
    const int Cc = std::min(512, st.out.Cpad - c0);
    const int threads = std::max(Cc, 256 / Cc * Cc);
    const int lanes = threads / Cc;
    int rc;
    if (det && (rc = grow_buf(s, &ts->det_part, &ts->det_part_bytes, (size_t)256 * st.out.Cpad * sizeof(float), false))) return rc;
    if (threads != lanes * Cc) BSMI_FAIL(BSMI_ERR_STATE, "column sums: block of %d threads for %d channels", threads, Cc);
    hipLaunchKernelGGL(colsum_kernel, dim3(256), dim3(threads), det ? (size_t)threads * sizeof(float) : 0, s, (const float*)cb.gp.ptr, st.out.D, st.out.H, st.out.W, st.out.Cpad, c0, Cc,
                       cb.P[0], cb.P[1], cb.P[2], p.cout, gb, gbr, det ? (float*)ts->det_part : (float*)nullptr);
    if (det) {  // the real channels of this chunk, rows in index order
      const int wd = std::min(Cc, p.cout - c0);
      if (wd > 0)
        hipLaunchKernelGGL(fold_kernel<float>, dim3((wd + 31) / 32), dim3(1024), 0, s, (const float*)ts->det_part + c0, 256, st.out.Cpad, wd,
                           gb + c0, gbr ? gbr + c0 : (float*)nullptr, 0);
    }
  }
  return BSMI_OK;
}

int launch_scatter(TrainState* ts, const ConvBwd& cb, hipStream_t s) {
  const PlanStep& st = *cb.st;
  const PassSite& p = *st.site;
  int cbase = 0;
  for (int sl = 0; sl < p.nslots; ++sl) {
    TDesc gt = ts->grad_of[st.slots[sl].ptr];
    if (!gt.ptr) BSMI_FAIL(BSMI_ERR_STATE, "training plan: no gradient tensor for an input of %s", p.prefix.c_str());
    const size_t total = (size_t)cb.dcat.D * cb.dcat.H * cb.dcat.W * p.cin[sl];
    hipLaunchKernelGGL(scatter_add_kernel, dim3(grid_1d(total, 16384)), dim3(256), 0, s, (const float*)cb.dcat.ptr, cb.dcat.D, cb.dcat.H, cb.dcat.W,
                       cb.dcat.Cpad, cbase, (float*)gt.ptr, gt.H, gt.W, gt.Cpad, 0, st.so[sl][0], st.so[sl][1], st.so[sl][2], p.cin[sl]);
    cbase += p.cin[sl];
  }
  return BSMI_OK;
}

void launch_adam(TrainState* ts, float lr, float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float gscale, hipStream_t s) {
  hipLaunchKernelGGL(adam_kernel, dim3(1024), dim3(256), 0, s, ts->w, (const float*)ts->g, ts->m, ts->v, ts->nparams, lr, beta1, beta2, eps, bc1,
                     bc2_sqrt, gscale);
}

}  // namespace bsmi

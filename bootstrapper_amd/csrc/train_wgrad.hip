// Training engine: weight gradients.  dW[n][c][tap] = sum over output voxels m of g[m][n] x[m + tap][c], g the stage's masked,
// padded gradient and x a source of its forward launch (train_internal.h has the file map and the stream rules: everything
// here runs on the weight gradients' stream).  Four kernel families:
//   wgrad_kernel<KX>             f32, one wave per 32 x 64 block of (n, c), operands straight from global memory
//   wgrad_tiled_kernel<KX>       f32, 128 x 128 block per workgroup through LDS (n and c both above 32)
//   wgrad_x3_kernel<KX,FNW,FCW>  split-bf16 on packed operands (wgrad_pack_kernel), sums into a tap-major workspace that
//                                wgrad_finish_kernel adds into the gradient buffer; chosen whenever the state has the workspace
//                                (TrainState::gt) and kx is 1 or 3
//   the same with per-line-range copies of the workspace and wgrad_finish_det_kernel: the deterministic mode
// The host side is WgradStage: the weight gradients of one conv stage, a weight tensor at a time (begin_tensor, one launch per
// source tensor, end_tensor), and launch_wgrad_stage, which runs it for a plan step.
#include <cstdlib>

#include "train_internal.h"

namespace bsmi {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8_t;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) char* wg_gptr_t;
typedef __attribute__((address_space(3))) char* wg_lptr_t;

// Weight gradient of one kernel tap: dW[n][cbase + c][tap] += sum over output voxels m of g[m][n] x[m + tap][c].
// One wave per (32 x 32 block of (n, c), tap, chunk of output lines); v_mfma_f32_32x32x2_f32 contracts two voxels per
// instruction, and since every lane of that instruction supplies ONE element (row lane % 32, k = lane / 32) both operands
// are read straight from the channels-last tensors: 32 lanes = 128 contiguous bytes of one voxel.
struct WgradArgs {
  const float* g; long long gsz, gsy, gsx;  // interior of the padded gradient: origin pointer and strides (floats)
  const float* x; long long xsz, xsy, xsx;  // source tensor at (slot origin + tap origin) and strides (floats)
  int Do, Ho, Wo;
  int N, C;            // real output / input channels of this slot
  int kz, ky, kx;      // taps of this launch (1,1,1 for the residual)
  float* dw;           // gradient of the weight [N][Cin_total][ntap]
  float* dwt;          // split-bf16 form: tap-major workspace [ntap][N][Cin_total] (wgrad_finish_kernel adds it into dw)
  int cin_total, cbase, ntap;
  int lines_per_block;
};

// KX = kx taps of one (kz, ky) tap row are accumulated by the same wave: one g value and KX pairs of x values per
// voxel pair feed 2 * KX MFMAs (a 32 x 64 block of (n, c) per tap); 96 accumulator registers, so several waves share
// a SIMD and hide each other's load latency.
template <int KX>
__global__ __launch_bounds__(64) void wgrad_kernel(const WgradArgs a) {
  const int lane = threadIdx.x, lr = lane & 31, lh = lane >> 5;
  const int nblocks_c = (a.C + 63) / 64;
  const int nb = blockIdx.x / nblocks_c, cb = blockIdx.x - nb * nblocks_c;
  const int trow = blockIdx.y;  // (tz, ty)
  const int tz = trow / a.ky, ty = trow - tz * a.ky;
  const int n0 = nb * 32 + lr, c0 = cb * 64 + lr;
  const bool nok0 = n0 < a.N, cok0 = c0 < a.C, cok1 = c0 + 32 < a.C;
  const float* gp = a.g + (nok0 ? n0 : 0);
  const float* xp = a.x + (cok0 ? c0 : 0) + tz * a.xsz + ty * a.xsy;
  f32x16_t acc[KX][2];
#pragma unroll
  for (int t = 0; t < KX; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][j][r] = 0.f;
  const int nlines = a.Do * a.Ho;
  const int l0 = blockIdx.z * a.lines_per_block, l1 = min(nlines, l0 + a.lines_per_block);
  for (int l = l0; l < l1; ++l) {
    const int z = l / a.Ho, y = l - z * a.Ho;
    const float* gl = gp + z * a.gsz + y * a.gsy;
    const float* xl = xp + z * a.xsz + y * a.xsy;
#pragma unroll 2
    for (int x0 = 0; x0 < a.Wo; x0 += 2) {
      const int xx = x0 + lh;
      const bool ok = xx < a.Wo;
      const float g0 = (ok && nok0) ? gl[xx * a.gsx] : 0.f;
      float x0v[KX], x1v[KX];
#pragma unroll
      for (int t = 0; t < KX; ++t) {
        x0v[t] = (ok && cok0) ? xl[(xx + t) * a.xsx] : 0.f;
        x1v[t] = (ok && cok1) ? xl[(xx + t) * a.xsx + 32] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < KX; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, x0v[t], acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, x1v[t], acc[t][1], 0, 0, 0);
      }
    }
  }
  // acc[r]: row (n) = (r & 3) + 8 (r >> 2) + 4 lh, column (c) = lr
#pragma unroll
  for (int t = 0; t < KX; ++t) {
    const int tap = trow * KX + t;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = cb * 64 + j * 32 + lr;
      if (c >= a.C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int nn = nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (nn < a.N && acc[t][j][r] != 0.f)
          atomicAdd(&a.dw[((size_t)nn * a.cin_total + a.cbase + c) * a.ntap + tap], acc[t][j][r]);
      }
    }
  }
}

// LDS-tiled form for the wide layers: a workgroup of 4 waves (2 x 2) owns a 128 x 128 block of (n, c) for the KX taps of
// one (kz, ky) tap row.  32 voxels of g ([32][128] floats) and the 32 + KX - 1 voxels of x they meet are staged in LDS
// once and shared by the four waves (a 3x smaller global read volume than the per-wave form, which is bound by it);
// the next chunk is fetched into registers while the current one is multiplied.
template <int KX>
__global__ __launch_bounds__(256) void wgrad_tiled_kernel(const WgradArgs a) {
  constexpr int MB = 32, TW = 128, XR = MB + KX - 1;
  __shared__ float gs[MB][TW];
  __shared__ float xs[XR][TW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int wn = wave >> 1, wc = wave & 1;
  const int nblocks_c = (a.C + TW - 1) / TW;
  const int nt = blockIdx.x / nblocks_c, ct = blockIdx.x - nt * nblocks_c;
  const int trow = blockIdx.y;
  const int tz = trow / a.ky, ty = trow - tz * a.ky;
  const int nbase = nt * TW, cbase = ct * TW;
  // which of this wave's 2 x 2 blocks hold real channels (uniform)
  bool nuse[2], cuse[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    nuse[i] = nbase + wn * 64 + i * 32 < a.N;
    cuse[i] = cbase + wc * 64 + i * 32 < a.C;
  }
  f32x16_t acc[KX][2][2];
#pragma unroll
  for (int t = 0; t < KX; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][i][j][r] = 0.f;
  // staging: thread -> (row, 4-float column group); g: MB rows x 32 groups = 1024 float4 = 4 per thread; x: XR rows
  constexpr int GV = MB * (TW / 4) / 256, XV = (XR * (TW / 4) + 255) / 256;
  float4 gr[GV], xr[XV];
  const float* gp0 = a.g;
  const float* xp0 = a.x + tz * a.xsz + ty * a.xsy;
  const int nlines = a.Do * a.Ho;
  const int l0 = blockIdx.z * a.lines_per_block, l1 = min(nlines, l0 + a.lines_per_block);
  const int chunks_per_line = (a.Wo + MB - 1) / MB;
  const int nchunks = (l1 - l0) * chunks_per_line;
  auto fetch = [&](int ch) {
    const int l = l0 + ch / chunks_per_line, x0 = (ch % chunks_per_line) * MB;
    const int z = l / a.Ho, y = l - z * a.Ho;
    const float* gl = gp0 + z * a.gsz + y * a.gsy;
    const float* xl = xp0 + z * a.xsz + y * a.xsy;
#pragma unroll
    for (int v = 0; v < GV; ++v) {
      const int idx = tid + v * 256, row = idx / (TW / 4), c4 = (idx % (TW / 4)) * 4;
      const int xx = x0 + row, n = nbase + c4;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (xx < a.Wo && n < a.N) {  // channel counts are padded to 16, so a 4-group never straddles the tensor's row end
        val = *(const float4*)(gl + (long long)xx * a.gsx + n);
        if (n + 3 >= a.N) {
          if (n + 1 >= a.N) val.y = 0.f;
          if (n + 2 >= a.N) val.z = 0.f;
          val.w = 0.f;
        }
      }
      gr[v] = val;
    }
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int idx = tid + v * 256, row = idx / (TW / 4), c4 = (idx % (TW / 4)) * 4;
      const int xx = x0 + row, c = cbase + c4;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < XR && xx < a.Wo + KX - 1 && c < a.C) {
        val = *(const float4*)(xl + (long long)xx * a.xsx + c);
        if (c + 3 >= a.C) {
          if (c + 1 >= a.C) val.y = 0.f;
          if (c + 2 >= a.C) val.z = 0.f;
          val.w = 0.f;
        }
      }
      xr[v] = val;
    }
  };
  if (nchunks > 0) fetch(0);
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // the previous chunk has been multiplied
#pragma unroll
    for (int v = 0; v < GV; ++v) {
      const int idx = tid + v * 256;
      *(float4*)&gs[idx / (TW / 4)][(idx % (TW / 4)) * 4] = gr[v];
    }
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int idx = tid + v * 256;
      if (idx / (TW / 4) < XR) *(float4*)&xs[idx / (TW / 4)][(idx % (TW / 4)) * 4] = xr[v];
    }
    __syncthreads();
    if (ch + 1 < nchunks) fetch(ch + 1);
    const int x0 = (ch % chunks_per_line) * MB;
    const int mvalid = min(MB, a.Wo - x0);  // rows beyond hold zeros in gs (fetch), so they add nothing
#pragma unroll 4
    for (int m = 0; m < MB; m += 2) {
      if (m >= mvalid) break;
      float g2[2], x2[KX][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) g2[i] = gs[m + lh][wn * 64 + i * 32 + lr];
#pragma unroll
      for (int t = 0; t < KX; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) x2[t][j] = xs[m + lh + t][wc * 64 + j * 32 + lr];
#pragma unroll
      for (int t = 0; t < KX; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            if (nuse[i] && cuse[j]) acc[t][i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(g2[i], x2[t][j], acc[t][i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < KX; ++t) {
    const int tap = trow * KX + t;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = cbase + wc * 64 + j * 32 + lr;
        if (!nuse[i] || c >= a.C) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int nn = nbase + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (nn < a.N && acc[t][i][j][r] != 0.f) atomicAdd(&a.dw[((size_t)nn * a.cin_total + a.cbase + c) * a.ntap + tap], acc[t][i][j][r]);
        }
      }
  }
}

// ---- split-bf16 weight gradient -------------------------------------------------------------------------------------
// The same sums on the bf16 matrix pipe (16x the rate of v_mfma_f32_32x32x2_f32): every f32 operand is split into
// hi = bf16(v), lo = bf16(v - hi) and the product is hi*hi + lo*hi + hi*lo with f32 accumulation (what BSMI_PREC_BF16X3
// does in the forward pass; relative error ~2^-17 per product).  v_mfma_f32_16x16x32_bf16 contracts 32 voxels per
// instruction and wants 8 consecutive K values (voxels) of one row (channel) per lane -- the transpose of the channels-last
// tensors.  So the operands are PACKED first (wgrad_pack_kernel, one elementwise pass per operand and conv stage):
//   G[group][plane][channel][8]   group = 8 consecutive output voxels of a line (the last group of a line zero-filled),
//                                 plane = hi | lo, channels padded to the tile; one more all-zero group at the end
//   X[group][plane][vec][channel][8]   the 8 input voxels under the group and, in vec 1, the next 8 (KX > 1): the operand
//                                 of kernel tap t is the group's vector shifted by t values
// so that 64 channels of one (group, plane) are 1 KiB of contiguous memory = ONE LDS-DMA instruction, and the fragments
// are plain 16-byte LDS reads.  (The first version split the f32 tensors inside the kernel: ~10 VALU instructions per
// element loaded left the MFMA pipe idle 80 % of the time.)
// A chunk = 4 groups = the K = 32 of one MFMA (19-voxel lines fill 79 % of the slots; whole-line chunks would fill 59 %).
// A workgroup of 2 x 2 waves owns a (32 FNW) x (32 FCW) block of (n, c) for the KX taps of one (kz, ky) tap row and a
// range of output lines; wave w stages group w of every chunk; two LDS buffers: chunk ch + 1 lands while ch is multiplied.
// src: f32 tensor at its first (line, voxel) with strides in floats; lines = nz x ny lines of `width` valid voxels, `gpl`
// groups per line; dst[((group * 2 + plane) * nvec + vec) * cpad + c] = 16-byte vector of voxels 8 (xg + vec) .. + 7 of
// channel c (zeros past `width` and past `creal`); `nullg` more all-zero groups follow.
__global__ void wgrad_pack_kernel(const float* __restrict__ src, long long sz, long long sy, long long sx, int nz, int ny, int width, int creal,
                                  int cpad, int gpl, int nvec, int nullg, u32x4_t* __restrict__ dst) {
  // 32-bit index arithmetic (the host checks the item count): 64-bit divisions cost more than the rest of the body
  const uint32_t ngroups = (uint32_t)nz * ny * gpl;
  const uint32_t total = (ngroups + nullg) * cpad;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t grp = i / (uint32_t)cpad;
    const int c = (int)(i - grp * cpad);
    const uint32_t line = grp / (uint32_t)gpl;
    const int xg = (int)(grp - line * gpl);
    const int z = (int)(line / (uint32_t)ny), y = (int)(line - (uint32_t)z * ny);
    const bool ok = grp < ngroups && c < creal;
    const float* sp = src + (ok ? (long long)z * sz + (long long)y * sy + c : 0);
    for (int v = 0; v < nvec; ++v) {
      u32x4_t hi, lo;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int x0 = (xg + v) * 8 + 2 * d;
        const float f0 = (ok && x0 < width) ? sp[x0 * sx] : 0.f;
        const float f1 = (ok && x0 + 1 < width) ? sp[(x0 + 1) * sx] : 0.f;
        uint32_t h, l;
        split_pair(f0, f1, h, l);
        hi[d] = h;
        lo[d] = l;
      }
      dst[(((size_t)grp * 2 + 0) * nvec + v) * cpad + c] = hi;
      dst[(((size_t)grp * 2 + 1) * nvec + v) * cpad + c] = lo;
    }
  }
}

struct WgradPk {
  const char* gp;  // packed g: [ngroups + 1][2][Np][16 B]
  const char* xp;  // packed x: [input lines * gpl][2][XVEC][Cp][16 B]
  int Np, Cp, gpl;
  int Do, Ho, Hil;  // output lines Do x Ho; input lines per z: Ho + ky - 1
  int N, C;         // real channels
  int kz, ky;
  float* dwt;       // tap-major workspace [ntap][N][cin_total]
  int cin_total, cbase, ntap;
  int lines_per_block, zsplit;
  size_t zstride;   // deterministic mode: line range z adds into its own copy of the workspace, dwt + z * zstride (0: one copy)
};

template <int KX, int FNW, int FCW>
__global__ __launch_bounds__(256, 2) void wgrad_x3_kernel(const WgradPk a) {
  // (two workgroups per CU: at most 96 accumulator registers per lane.  The 128 x 128 tile's 192 did not fit beside the
  // operands: the compiler shuttled fragments through AGPRs, 350 copies per chunk, and one wave per SIMD hid nothing)
  constexpr int TN = 32 * FNW, TC = 32 * FCW;
  static_assert(KX * FNW * FCW * 4 <= 96, "accumulators");
  constexpr int XVEC = KX > 1 ? 2 : 1;
  constexpr int GBYTES = 2 * 4 * TN * 16;          // [plane][group][TN][16 B]
  constexpr int XBYTES = 2 * XVEC * 4 * TC * 16;   // [plane][vec][group][TC][16 B]
  constexpr int BUF = GBYTES + XBYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // two buffers
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wc = wave & 1;
  // Workgroup -> (tile, line range, tap row), XCD-aware: consecutive workgroup ids go round-robin to the 8 XCDs, so the
  // kz * ky tap rows of one (tile, line range) are made consecutive ON one XCD: they run together and share the tile's
  // g vectors and (shifted by a line or two) x vectors in that XCD's L2 (id-major order sent the 9 readers of the same
  // vectors to different XCDs at different times: 3.9 TB/s of L2 misses on the 1500 -> 1500 layer).
  const int nblocks_c = (a.C + TC - 1) / TC;
  const int ntiles = ((a.N + TN - 1) / TN) * nblocks_c;
  const int trows = a.kz * a.ky;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int trow = seq % trows;
  const int unit = (seq / trows) * 8 + xcd;
  if (unit >= ntiles * a.zsplit) return;  // (uniform; the grid is padded to 8 x trows)
  const int tile = unit % ntiles, zblk = unit / ntiles;
  // deterministic mode: this line range's own copy of the workspace -- one contributor per element, wgrad_finish_kernel adds the
  // copies in z order (the atomicAdd below then adds to a zero and is exact whatever the order of the workgroups)
  float* const dwt_z = a.dwt + (size_t)zblk * a.zstride;
  const int nt = tile / nblocks_c, ct = tile - nt * nblocks_c;
  const int tz = trow / a.ky, ty = trow - tz * a.ky;
  const int nbase = nt * TN, cbase = ct * TC;
  bool nuse[FNW], cuse[FCW];
#pragma unroll
  for (int i = 0; i < FNW; ++i) nuse[i] = nbase + (wn * FNW + i) * 16 < a.N;
#pragma unroll
  for (int j = 0; j < FCW; ++j) cuse[j] = cbase + (wc * FCW + j) * 16 < a.C;
  const bool nall = nuse[FNW - 1];
  f32x4_t acc[KX][FNW][FCW];
#pragma unroll
  for (int t = 0; t < KX; ++t)
#pragma unroll
    for (int i = 0; i < FNW; ++i)
#pragma unroll
      for (int j = 0; j < FCW; ++j) acc[t][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int gpl = a.gpl;
  const int nlines = a.Do * a.Ho;
  const int l0 = zblk * a.lines_per_block, l1 = min(nlines, l0 + a.lines_per_block);
  const int ngroups = (l1 - l0) * gpl;
  const int nchunks = (ngroups + 3) >> 2;
  // this wave's group of the chunk being staged: index within the block's range, output line (z, y), group of the line
  int gi = wave, pz, py, pxg;
  {
    const int line = l0 + wave / gpl;
    pxg = wave % gpl;
    pz = line / a.Ho;
    py = line - pz * a.Ho;
  }
  const size_t gvec = (size_t)a.Np * 16, xvec = (size_t)a.Cp * 16;  // bytes of one (group, plane[, vec]) row of all channels
  const wg_gptr_t gsrc = (wg_gptr_t)a.gp + (size_t)(nbase + lane) * 16;
  const wg_gptr_t xsrc = (wg_gptr_t)a.xp + (size_t)(cbase + lane) * 16;
  const size_t gnull = (size_t)nlines * gpl;  // the all-zero group
  auto stage = [&](int buf) __attribute__((always_inline)) {
    const bool ok = gi < ngroups;
    const size_t gabs = ok ? (size_t)l0 * gpl + gi : gnull;
    const size_t xabs = ok ? ((size_t)(pz + tz) * a.Hil + (py + ty)) * gpl + pxg : 0;  // past the range: any group (g is zero)
    const wg_lptr_t lg = (wg_lptr_t)(smem + buf * BUF);
    const wg_lptr_t lx = (wg_lptr_t)(smem + buf * BUF + GBYTES);
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      // one instruction = 64 channels of a (group, plane); a 32-channel tile uses the lower half of the lanes
#pragma unroll
      for (int hf = 0; hf < (TN + 63) / 64; ++hf)
        if (TN >= 64 || lane < TN)
          __builtin_amdgcn_global_load_lds(gsrc + (gabs * 2 + pl) * gvec + hf * 1024, lg + ((pl * 4 + wave) * TN + hf * 64) * 16, 16, 0, 0);
#pragma unroll
      for (int v = 0; v < XVEC; ++v)
#pragma unroll
        for (int hf = 0; hf < (TC + 63) / 64; ++hf)
          if (TC >= 64 || lane < TC)
            __builtin_amdgcn_global_load_lds(xsrc + ((xabs * 2 + pl) * XVEC + v) * xvec + hf * 1024,
                                             lx + (((pl * XVEC + v) * 4 + wave) * TC + hf * 64) * 16, 16, 0, 0);
    }
    // four groups on
    gi += 4;
    pxg += 4;
    while (pxg >= gpl) {
      pxg -= gpl;
      if (++py == a.Ho) { py = 0; ++pz; }
    }
  };
  auto mfma = [](f32x4_t c, u32x4_t x, u32x4_t y) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x), __builtin_bit_cast(bf16x8_t, y), c, 0, 0, 0);
  };
  const uint32_t aoff = (uint32_t)((lq * TN + wn * FNW * 16 + lr) * 16);
  const uint32_t boff = (uint32_t)((lq * TC + wc * FCW * 16 + lr) * 16);
  if (nchunks > 0) stage(0);
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's group of chunk ch has landed
    __syncthreads();                                  // ... everybody's has, and chunk ch - 1 has been multiplied
    if (ch + 1 < nchunks) stage(buf ^ 1);
    const char* gs = smem + buf * BUF;
    const char* xs = gs + GBYTES;
    u32x4_t ah[FNW], al[FNW];
#pragma unroll
    for (int i = 0; i < FNW; ++i) {
      ah[i] = *(const u32x4_t*)(gs + aoff + i * 256);
      al[i] = *(const u32x4_t*)(gs + 4 * TN * 16 + aoff + i * 256);
    }
#pragma unroll
    for (int j = 0; j < FCW; ++j) {
      if (!cuse[j]) continue;
      uint32_t d[2][5];
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const char* xb = xs + pl * XVEC * 4 * TC * 16 + boff + j * 256;
        const u32x4_t q = *(const u32x4_t*)xb;
        d[pl][0] = q.x; d[pl][1] = q.y; d[pl][2] = q.z; d[pl][3] = q.w;
        d[pl][4] = XVEC > 1 ? *(const uint32_t*)(xb + 4 * TC * 16) : 0u;
      }
      u32x4_t bh[KX], bl[KX];
#pragma unroll
      for (int t = 0; t < KX; ++t) {
        u32x4_t qh, ql;
        if (t == 0) {
          qh = u32x4_t{d[0][0], d[0][1], d[0][2], d[0][3]};
          ql = u32x4_t{d[1][0], d[1][1], d[1][2], d[1][3]};
        } else if (t == 1) {
          qh = u32x4_t{__builtin_amdgcn_alignbyte(d[0][1], d[0][0], 2), __builtin_amdgcn_alignbyte(d[0][2], d[0][1], 2),
                       __builtin_amdgcn_alignbyte(d[0][3], d[0][2], 2), __builtin_amdgcn_alignbyte(d[0][4], d[0][3], 2)};
          ql = u32x4_t{__builtin_amdgcn_alignbyte(d[1][1], d[1][0], 2), __builtin_amdgcn_alignbyte(d[1][2], d[1][1], 2),
                       __builtin_amdgcn_alignbyte(d[1][3], d[1][2], 2), __builtin_amdgcn_alignbyte(d[1][4], d[1][3], 2)};
        } else {
          qh = u32x4_t{d[0][1], d[0][2], d[0][3], d[0][4]};
          ql = u32x4_t{d[1][1], d[1][2], d[1][3], d[1][4]};
        }
        bh[t] = qh;
        bl[t] = ql;
      }
      // three products per accumulator, the accumulators of a product back to back (independent instructions)
      // (a wave whose n fragments are all real -- every wave but those of a layer's last tile -- runs them without a branch)
      if (nall) {
#pragma unroll
        for (int pr = 0; pr < 3; ++pr)
#pragma unroll
          for (int t = 0; t < KX; ++t)
#pragma unroll
            for (int i = 0; i < FNW; ++i) acc[t][i][j] = mfma(acc[t][i][j], pr == 1 ? al[i] : ah[i], pr == 2 ? bl[t] : bh[t]);
      } else {
#pragma unroll
        for (int i = 0; i < FNW; ++i) {
          if (!nuse[i]) continue;
#pragma unroll
          for (int pr = 0; pr < 3; ++pr)
#pragma unroll
            for (int t = 0; t < KX; ++t) acc[t][i][j] = mfma(acc[t][i][j], pr == 1 ? al[i] : ah[i], pr == 2 ? bl[t] : bh[t]);
        }
      }
    }
  }
  // acc[r]: row (n) = 4 (lane >> 4) + r, column (c) = lane & 15
#pragma unroll
  for (int t = 0; t < KX; ++t) {
    const int tap = trow * KX + t;
#pragma unroll
    for (int i = 0; i < FNW; ++i)
#pragma unroll
      for (int j = 0; j < FCW; ++j) {
        const int c = cbase + (wc * FCW + j) * 16 + lr;
        if (!nuse[i] || !cuse[j] || c >= a.C) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nn = nbase + (wn * FNW + i) * 16 + 4 * lq + r;
          // tap-major: the 16 lanes of a row are 64 contiguous bytes (in the OIDHW gradient they are 4 ntap bytes apart,
          // one cache line per lane)
          if (nn < a.N && acc[t][i][j][r] != 0.f) atomicAdd(&dwt_z[((size_t)tap * a.N + nn) * a.cin_total + a.cbase + c], acc[t][i][j][r]);
        }
      }
  }
}

// dw[n][c][tap] += dwt[tap][n][c]; dwt = 0 (ready for the next step).  A block takes 256 consecutive (n, c): the tap planes
// are read coalesced over (n, c), transposed through LDS and added into the OIDHW gradient as one contiguous run.
// nz, zstride (deterministic mode): the workspace is nz copies, one per line range of the launches; they are added in z order.
__global__ __launch_bounds__(256) void wgrad_finish_kernel(float* __restrict__ dwt, float* __restrict__ dw, size_t nc, int ntap, int nz,
                                                           size_t zstride) {
  __shared__ float tile[256 * 28];
  const size_t i0 = (size_t)blockIdx.x * 256;
  const int n = (int)min((size_t)256, nc - i0);
  const int tid = threadIdx.x;
  auto take = [&](int t) -> float {  // the sum over the copies, each left zero
    float acc = 0.f;
    for (int z = 0; z < nz; ++z) {
      float* q = dwt + (size_t)z * zstride + (size_t)t * nc + i0 + tid;
      const float v = *q;
      if (v != 0.f) { acc += v; *q = 0.f; }
    }
    return acc;
  };
  if (ntap > 27) {  // (no such kernel in the model family; plain form)
    if (tid < n)
      for (int t = 0; t < ntap; ++t) {
        const float v = take(t);
        if (v != 0.f) dw[(i0 + tid) * ntap + t] += v;
      }
    return;
  }
  if (tid < n)
    for (int t = 0; t < ntap; ++t) tile[tid * 28 + t] = take(t);
  __syncthreads();
  const int total = n * ntap;
  float* d = dw + i0 * ntap;
  for (int k = tid; k < total; k += 256) {
    const int i = k / ntap, t = k - i * ntap;
    const float v = tile[i * 28 + t];
    if (v != 0.f) d[k] += v;
  }
}

// The same for the deterministic mode's nz copies: 1024 threads = 256 (n, c) x 4 tap groups (a narrow layer is ONE workgroup here
// and its launches were cut into many line ranges: 27 taps x nz dependent loads per thread took milliseconds); four copies are in
// flight at a time and are added in z order.
constexpr int kDetMaxRanges = 32;  // line ranges per launch in the deterministic mode (launch_wgrad_x3_t)
__global__ __launch_bounds__(1024) void wgrad_finish_det_kernel(float* __restrict__ dwt, float* __restrict__ dw, size_t nc, int ntap, int nz,
                                                                size_t zstride) {
  __shared__ float tile[256 * 28];
  const size_t i0 = (size_t)blockIdx.x * 256;
  const int n = (int)min((size_t)256, nc - i0);
  const int tid = threadIdx.x & 255, tg = threadIdx.x >> 8;
  if (tid < n)
    for (int t = tg; t < ntap; t += 4) {
      float* q = dwt + (size_t)t * nc + i0 + tid;
      float acc = 0.f;
      int z = 0;
      for (; z + 3 < nz; z += 4) {
        float* q0 = q + (size_t)z * zstride;
        const float v0 = q0[0], v1 = q0[zstride], v2 = q0[2 * zstride], v3 = q0[3 * zstride];
        acc += v0; acc += v1; acc += v2; acc += v3;
        if (v0 != 0.f) q0[0] = 0.f;
        if (v1 != 0.f) q0[zstride] = 0.f;
        if (v2 != 0.f) q0[2 * zstride] = 0.f;
        if (v3 != 0.f) q0[3 * zstride] = 0.f;
      }
      for (; z < nz; ++z) {
        float* q0 = q + (size_t)z * zstride;
        const float v = *q0;
        acc += v;
        if (v != 0.f) *q0 = 0.f;
      }
      tile[tid * 28 + t] = acc;
    }
  __syncthreads();
  const int total = n * ntap;
  float* d = dw + i0 * ntap;
  for (int k = threadIdx.x; k < total; k += 1024) {
    const int i = k / ntap, t = k - i * ntap;
    const float v = tile[i * 28 + t];
    if (v != 0.f) d[k] += v;
  }
}

// tile widths the launcher picks (= channel padding of the packed operands): 32 / 64 / 128 output channels x 32 / 64
// input channels
static int wgrad_tile_n(int n) { return n <= 32 ? 32 : (n <= 64 ? 64 : 128); }
static int wgrad_tile_c(int c) { return c <= 32 ? 32 : 64; }
static int wgrad_pad(int channels, int tile) { return (channels + tile - 1) / tile * tile; }

template <int KX, int FNW, int FCW>
static int launch_wgrad_x3_t(WgradPk a, hipStream_t s, bsmi_unet_train_wgrad_info* wi) {
  constexpr int TN = 32 * FNW, TC = 32 * FCW, XVEC = KX > 1 ? 2 : 1;
  constexpr int smem = 2 * (2 * 4 * TN * 16 + 2 * XVEC * 4 * TC * 16);
  static DeviceOnce once;
  const int rc_once = once.run([&]() -> int {
    BSMI_HIP(hipFuncSetAttribute((const void*)wgrad_x3_kernel<KX, FNW, FCW>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    return BSMI_OK;
  });
  if (rc_once) return rc_once;
  const int nlines = a.Do * a.Ho, trows = a.kz * a.ky;
  const int blocks_nc = ((a.N + TN - 1) / TN) * ((a.C + TC - 1) / TC);
  int zsplit = std::max(1, std::min(nlines, 4096 / std::max(1, blocks_nc * trows)));
  if (a.zstride) zsplit = std::min(zsplit, kDetMaxRanges);
  const int zcap = a.zsplit;  // deterministic mode: the copies of the workspace the caller has room for
  a.lines_per_block = (nlines + zsplit - 1) / zsplit;
  a.zsplit = (nlines + a.lines_per_block - 1) / a.lines_per_block;
  if (a.zstride && a.zsplit > zcap) BSMI_FAIL(BSMI_ERR_STATE, "weight-gradient launch cut into %d line ranges, workspace for %d", a.zsplit, zcap);
  const int units = blocks_nc * a.zsplit;
  if (wi) {  // (bsmi_unet_train_debug_step_info)
    wi->family = BSMI_WGRAD_SPLIT; wi->kx = KX; wi->tile_n = TN; wi->tile_c = TC;
    wi->ranges = a.zsplit; wi->lines_per_range = a.lines_per_block; wi->det_workspace = a.zstride ? 1 : 0;
  }
  hipLaunchKernelGGL((wgrad_x3_kernel<KX, FNW, FCW>), dim3((units + 7) / 8 * 8 * trows), dim3(256), smem, s, a);
  return BSMI_OK;
}

template <int KX>
static int launch_wgrad_x3_k(const WgradPk& a, hipStream_t s, bsmi_unet_train_wgrad_info* wi) {
  const int fn = wgrad_tile_n(a.N) / 32, fc = wgrad_tile_c(a.C) / 32;
  if (fn == 1 && fc == 1) return launch_wgrad_x3_t<KX, 1, 1>(a, s, wi);
  if (fn == 1 && fc == 2) return launch_wgrad_x3_t<KX, 1, 2>(a, s, wi);
  if (fn == 2 && fc == 1) return launch_wgrad_x3_t<KX, 2, 1>(a, s, wi);
  if (fn == 2 && fc == 2) return launch_wgrad_x3_t<KX, 2, 2>(a, s, wi);
  if (fn == 4 && fc == 1) return launch_wgrad_x3_t<KX, 4, 1>(a, s, wi);
  return launch_wgrad_x3_t<KX, 4, 2>(a, s, wi);
}

// the line ranges launch_wgrad_x3_t will cut a slot's launch into (its arithmetic)
static int wgrad_x3_ranges(int N, int C, int nlines, int trows) {
  const int TN = wgrad_tile_n(N), TC = wgrad_tile_c(C);
  const int blocks_nc = ((N + TN - 1) / TN) * ((C + TC - 1) / TC);
  const int zs = std::min(kDetMaxRanges, std::max(1, std::min(nlines, 4096 / std::max(1, blocks_nc * trows))));
  const int lpb = (nlines + zs - 1) / zs;
  return (nlines + lpb - 1) / lpb;
}

// The weight gradients of one conv stage.  A stage has one weight tensor, its last stage also the pass's residual weight; a
// tensor takes one launch per source tensor of the forward launch (two where the pass input is a concatenation), each adding
// into its own range [cbase, cbase + C) of the tensor's input channels.
struct WgradStage {
  TrainState* ts;
  hipStream_t sw;
  bool det;
  bsmi_unet_train_step_info* ri;  // the step's record: one bsmi_unet_train_wgrad_info per launch, up to 4
  // the stage: interior of its padded gradient, output extent, output channels
  const float* g;
  int64_t gsz, gsy, gsx;
  int Do, Ho, Wo, N;
  bool g_packed = false;  // pk_g holds this stage's g: packed by the stage's first split-bf16 launch, reused by the residual tensor's
  // the weight tensor whose launches are being issued (begin_tensor .. end_tensor)
  float* dw = nullptr;    // its gradient, [N][cin_total][ntap]
  int cin_total = 0, k[3] = {1, 1, 1}, ntap = 1;
  bool residual = false;
  bool split = false;     // its launches take the split-bf16 form (and end_tensor has a workspace to fold)
  // deterministic mode: the launches of one weight tensor add into per-line-range copies of its workspace (det_nz of them,
  // det_numel floats apart, in ts->gt_det), which the finish kernel adds in order
  int det_nz = 1;
  size_t det_numel = 0;

  WgradStage(TrainState* ts_, size_t step, bool det_, hipStream_t sw_) : ts(ts_), sw(sw_), det(det_), ri(&ts_->rec[step]) {
    const ConvBwd& cb = ts->convs[step];
    gsx = cb.gp.Cpad; gsy = (int64_t)cb.gp.W * gsx; gsz = (int64_t)cb.gp.H * gsy;
    g = (const float*)cb.gp.ptr + cb.P[0] * gsz + cb.P[1] * gsy + cb.P[2] * gsx;
    Do = cb.st->out.D; Ho = cb.st->out.H; Wo = cb.st->out.W;
    N = cb.st->site->cout;
  }

  // before the launches of one weight tensor; slot_c: the channels of its nsl sources
  int begin_tensor(const ParamRef* w, int cin_total_, const int* k_, bool residual_, const int* slot_c, int nsl) {
    dw = ts->g + w->off;
    cin_total = cin_total_;
    for (int d = 0; d < 3; ++d) k[d] = k_[d];
    ntap = k[0] * k[1] * k[2];
    residual = residual_;
    split = ts->gt && (k[2] == 1 || k[2] == 3);
    if (!det || !ts->gt) return BSMI_OK;
    det_numel = (size_t)ntap * N * cin_total;
    det_nz = 1;
    for (int sl = 0; sl < nsl; ++sl) det_nz = std::max(det_nz, wgrad_x3_ranges(N, slot_c[sl], Do * Ho, k[0] * k[1]));
    return grow_buf(sw, &ts->gt_det, &ts->gt_det_bytes, (size_t)det_nz * det_numel * sizeof(float), true);
  }

  // one source: x at voxel origin org, C channels that are channels [cbase, cbase + C) of the weight
  int launch(const TDesc& x, const int* org, int C, int cbase) {
    WgradArgs a;
    a.g = g; a.gsz = gsz; a.gsy = gsy; a.gsx = gsx;
    a.xsx = x.Cpad; a.xsy = (int64_t)x.W * a.xsx; a.xsz = (int64_t)x.H * a.xsy;
    a.x = (const float*)x.ptr + org[0] * a.xsz + org[1] * a.xsy + org[2] * a.xsx;
    a.Do = Do; a.Ho = Ho; a.Wo = Wo;
    a.N = N; a.C = C;
    a.kz = k[0]; a.ky = k[1]; a.kx = k[2];
    a.dw = dw; a.cin_total = cin_total; a.cbase = cbase; a.ntap = ntap;
    a.dwt = ts->gt ? ts->gt + (dw - ts->g) : nullptr;
    const int nlines = a.Do * a.Ho;
    const int trows = a.kz * a.ky;
    bsmi_unet_train_wgrad_info* wi = ri->n_wgrad < 4 ? &ri->wgrad[ri->n_wgrad++] : nullptr;  // the record of this launch
    if (wi) {
      wi->residual = ntap == 1 && residual ? 1 : 0;
      wi->n = a.N; wi->c = a.C; wi->cbase = a.cbase;
    }
    if (split) return launch_split(a, wi);
    const bool tiled = a.N > 32 && a.C > 32;  // narrow layers: the per-wave form wastes fewer MFMAs on padding
    const int blocks_nc = tiled ? ((a.N + 127) / 128) * ((a.C + 127) / 128) : ((a.N + 31) / 32) * ((a.C + 63) / 64);
    int zsplit = std::max(1, std::min(nlines, (tiled ? 2048 : 8192) / std::max(1, blocks_nc * trows)));
    if (det) zsplit = 1;  // the f32 forms add straight into dw: one workgroup per element = one (exact) addition to a zero
    a.lines_per_block = (nlines + zsplit - 1) / zsplit;
    zsplit = (nlines + a.lines_per_block - 1) / a.lines_per_block;
    const dim3 grid(blocks_nc, trows, zsplit);
    if (wi && a.kx >= 1 && a.kx <= 3) {
      wi->family = tiled ? BSMI_WGRAD_TILED_F32 : BSMI_WGRAD_WAVE_F32;
      wi->kx = a.kx; wi->tile_n = tiled ? 128 : 32; wi->tile_c = tiled ? 128 : 64;
      wi->ranges = zsplit; wi->lines_per_range = a.lines_per_block;
    }
    void (*const tiled_k[3])(WgradArgs) = {wgrad_tiled_kernel<1>, wgrad_tiled_kernel<2>, wgrad_tiled_kernel<3>};
    void (*const wave_k[3])(WgradArgs) = {wgrad_kernel<1>, wgrad_kernel<2>, wgrad_kernel<3>};
    if (a.kx < 1 || a.kx > 3) return BSMI_OK;  // (none: checked in bsmi_unet_train_begin)
    hipLaunchKernelGGL(tiled ? tiled_k[a.kx - 1] : wave_k[a.kx - 1], grid, dim3(tiled ? 256 : 64), 0, sw, a);
    return BSMI_OK;
  }

  // split-bf16 form (wgrad_x3_kernel): pack g once per conv stage, x per launch
  int launch_split(const WgradArgs& a, bsmi_unet_train_wgrad_info* wi) {
    const int gpl = (a.Wo + 7) / 8, nlines = a.Do * a.Ho;
    const int Np = wgrad_pad(a.N, wgrad_tile_n(a.N)), Cp = wgrad_pad(a.C, wgrad_tile_c(a.C)), xvec = a.kx > 1 ? 2 : 1;
    const int Dil = a.Do + a.kz - 1, Hil = a.Ho + a.ky - 1;
    int rc;
    if (!g_packed) {
      const size_t need = ((size_t)nlines * gpl + 1) * 2 * Np * 16;
      if ((rc = grow_buf(sw, &ts->pk_g, &ts->pk_g_bytes, need, false))) return rc;  // first steps only
      const size_t items = ((size_t)nlines * gpl + 1) * Np;
      if (items >= ((size_t)1 << 31)) return BSMI_ERR_INVALID;
      hipLaunchKernelGGL(wgrad_pack_kernel, dim3(grid_1d(items, 65536)), dim3(256), 0, sw, a.g, a.gsz, a.gsy, a.gsx, a.Do, a.Ho, a.Wo, a.N, Np, gpl, 1,
                         1, (u32x4_t*)ts->pk_g);
      g_packed = true;
    }
    const size_t needx = (size_t)Dil * Hil * gpl * 2 * xvec * Cp * 16;
    if ((rc = grow_buf(sw, &ts->pk_x, &ts->pk_x_bytes, needx, false))) return rc;
    const size_t itemsx = (size_t)Dil * Hil * gpl * Cp;
    if (itemsx >= ((size_t)1 << 31)) return BSMI_ERR_INVALID;
    hipLaunchKernelGGL(wgrad_pack_kernel, dim3(grid_1d(itemsx, 65536)), dim3(256), 0, sw, a.x, a.xsz, a.xsy, a.xsx, Dil, Hil, a.Wo + a.kx - 1, a.C, Cp,
                       gpl, xvec, 0, (u32x4_t*)ts->pk_x);
    WgradPk k;
    k.gp = ts->pk_g; k.xp = ts->pk_x; k.Np = Np; k.Cp = Cp; k.gpl = gpl;
    k.Do = a.Do; k.Ho = a.Ho; k.Hil = Hil; k.N = a.N; k.C = a.C; k.kz = a.kz; k.ky = a.ky;
    k.dwt = det ? (float*)ts->gt_det : a.dwt; k.cin_total = a.cin_total; k.cbase = a.cbase; k.ntap = a.ntap; k.lines_per_block = 0; k.zsplit = 1;
    k.zstride = det ? det_numel : 0;
    if (det) k.zsplit = det_nz;
    return a.kx == 1 ? launch_wgrad_x3_k<1>(k, sw, wi) : launch_wgrad_x3_k<3>(k, sw, wi);
  }

  // after the launches of one weight tensor: the split-bf16 form's workspace into the gradient
  int end_tensor() {
    if (!split) return BSMI_OK;
    const size_t nc = (size_t)N * cin_total;
    if (det && ntap > 27) BSMI_FAIL(BSMI_ERR_INVALID, "deterministic weight gradients: kernels of at most 27 taps");
    if (det)
      hipLaunchKernelGGL(wgrad_finish_det_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(1024), 0, sw, (float*)ts->gt_det, dw, nc, ntap, det_nz,
                         det_numel);
    else
      hipLaunchKernelGGL(wgrad_finish_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, sw, ts->gt + (dw - ts->g), dw, nc, ntap, 1, (size_t)0);
    return BSMI_OK;
  }

  // a whole weight tensor: source sl is x[sl] at origin org[sl] with slot_c[sl] channels
  int tensor(const ParamRef* w, const int* k_, bool residual_, const TDesc* x, const int (*org)[3], const int* slot_c, int nsl) {
    int ct = 0;
    for (int sl = 0; sl < nsl; ++sl) ct += slot_c[sl];
    int rc = begin_tensor(w, ct, k_, residual_, slot_c, nsl);
    if (rc) return rc;
    int cbase = 0;
    for (int sl = 0; sl < nsl; ++sl) {
      if ((rc = launch(x[sl], org[sl], slot_c[sl], cbase))) return rc;
      cbase += slot_c[sl];
    }
    return end_tensor();
  }
};

int launch_wgrad_stage(TrainState* ts, size_t step, bool det, hipStream_t sw) {
  const ConvBwd& cb = ts->convs[step];
  const PlanStep& st = *cb.st;
  const PassSite& p = *st.site;
  const int ci = st.ci;
  WgradStage wg(ts, step, det, sw);
  // the stage's own weight: the pass's sources on its first stage, else the previous stage's output
  const int one_slot[1] = {p.cout};
  int rc = wg.tensor(cb.par.w, p.k[ci], false, st.slots, st.so, ci == 0 ? p.cin : one_slot, ci == 0 ? p.nslots : 1);
  if (rc || ci != p.nconv - 1) return rc;
  // last stage: the residual 1x1x1 weight reads the pass's sources at the centre of what the pass crops
  int crop[3];
  pass_crop(p, crop);
  const int first_slot = ci == 0 ? 0 : 1;
  const int ones[3] = {1, 1, 1};
  int org[2][3];
  for (int sl = 0; sl < p.nslots; ++sl)
    for (int d = 0; d < 3; ++d) org[sl][d] = st.so[first_slot + sl][d] + crop[d] / 2;
  return wg.tensor(cb.par.rw, ones, true, st.slots + first_slot, org, p.cin, p.nslots);
}

}  // namespace bsmi

// Blosc-1 frames of 1-byte items (the affinity / LSD chunks of `bs predict`), encoded ON THE DEVICE.
//
// blosc_dev.hip beside this file writes label volumes, whose byte planes are runs; its LZ4 blocks know offset 1 only.  Affinities
// are noisy values that saturate near 254/255 inside objects and drop at boundaries: what compresses in them is repeats at a
// distance.  This is an LZ4 match finder in a parallel form whose output is nevertheless ONE specified byte string (restated
// sequentially in tests/blosc_u8_ref.py and held byte-equal to it).
//
// Frame (c-blosc 1.x for typesize 1, as csrc/chunk_codec.cpp writes it): header {2, 1, flags, 1, nbytes, blocksize, cbytes}, flags
// 0x30 (lz4 format, blocks not split), blocksize min(32 768, nbytes), the last block may be short; block starts; per block a
// 4-byte length + one LZ4 block, or the block verbatim when LZ4 does not shrink it.  A frame that would not be smaller than
// nbytes + 16 is stored (flags 0x32: header + the chunk's bytes).
//
// The rule of the LZ4 block of b[0..n).  Position i has at most two candidates:
//   run    offset 1, length r(i) = the number of consecutive j >= i with b[j] == b[j-1] (i >= 1); a candidate from 5 bytes on.
//   table  positions go in groups of 256.  A table of 4096 entries is indexed by h(i) = (le32(b, i) * 2654435761) >> 20
//          (i + 4 <= n).  Every position of a group looks up c = table[h(i)] as the table stood after all EARLIER groups; then
//          the whole group enters itself, table[h] = max(table[h], i) (an LDS atomicMax: the result does not depend on order).
//          The match at offset i - c has the length of the common prefix of b[c..] and b[i..] cut at 68; a candidate from 4 on.
//          (Repeats at distances 2..255 inside a group are therefore not found: part of the rule.)
// No match starts beyond n - 12, every length is cut so that the match ends at or before n - 5 (LZ4's end-of-block rules); a
// match cut below its minimum is no candidate.  The longer candidate wins, offset 1 on equal length.  The parse is greedy from 0:
// at i, a winner of length L is emitted (literals since the last match, then the match) and the parse goes to i + L, else i + 1.
//
// Kernel 1, one workgroup of 256 threads per (chunk, block), everything out of LDS (146 KiB: the block 32, a u16 per position
// 64 -- bit 15 + run length, or the table match's offset --, a u8 per position 32, the table 16, scans 2):
//   0  gather the block from the strided source; run lengths by a backward sweep of each thread's 128 positions + a suffix-min
//   1  the groups in turn: look up, compare, choose; barrier; enter; barrier
//   2  the chain i -> next(i): each thread sweeps its segment backwards for the LAST chain position inside the segment of every
//      entry (u8 per position: 128 + table length where the position leaves the segment itself, else the index of the one that does)
//   3  one walk over the segments (one thread, three LDS reads per segment) finds each segment's entry
//   4  each thread follows the chain through its segment: prefix-max -> end of the last match before the segment, prefix sum of
//      the encoded sizes -> where the segment's sequences go; then the sequences are written, the closing literals by all.
// Kernel 2, one workgroup per chunk: where the blocks go, header, block starts.  Kernel 3, one workgroup per (chunk, block): the
// blocks packed back to back, or the stored frame's bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "../../include/bsmi_io.h"

namespace bsmi {
namespace {

constexpr int kBlock = 32 * 1024;        // Blosc block size (bytes) of the frames
constexpr int kSeg = kBlock / 256;       // positions per thread
constexpr int kSlot = kBlock + 4;        // scratch per block: length prefix + data
constexpr int kHashBits = 12;
constexpr int kMaxTableLen = 68, kMinRun = 5, kMinTable = 4;
constexpr int kMaxBlocks = 1024;         // blocks per chunk (kernel 2 sums the sizes of at most 4 per thread)
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kGeoBatch = 32;            // chunks whose geometry one launch carries in its arguments
// LDS of kernel 1
constexpr int kOffS = 0;                                  // the block (+ 16 bytes so that le32 may read the word behind)
constexpr int kOffA = kBlock + 16;                        // u16 per position
constexpr int kOffB = kOffA + 2 * kBlock;                 // u8 per position
constexpr int kOffT = kOffB + kBlock;                     // table
constexpr int kOffBuf = kOffT + 4 * (1 << kHashBits);     // scans
constexpr int kOffEnt = kOffBuf + 4 * 256;                // entries of the segments
constexpr int kLds = kOffEnt + 4 * 256;

struct DevChunksU8 {
  const uint8_t* src;
  long long sc, sz, sy;         // element strides of the source (x contiguous)
  const long long* origin;      // [n][4] first voxel of every chunk, relative to src
  const long long* extent;      // [n][4] voxels of the chunk that exist (the rest is fill = 0)
  int cc, cz, cy, cx;           // chunk shape
  unsigned chunk_bytes;
  int nblocks;                  // blocks per chunk
};

struct GeoBatch {
  long long v[kGeoBatch * 8];   // per chunk: origin[4], extent[4]
};

// the geometry travels in the launch's arguments: nothing of the caller's has to outlive the call
__global__ void geo_write_kernel(const GeoBatch g, int first, int count, int n_chunks, long long* __restrict__ geo) {
  const int t = threadIdx.x;
  if (t >= count * 8) return;
  const int c = first + t / 8, k = t % 8;
  geo[(k < 4 ? 0 : (size_t)n_chunks * 4) + (size_t)c * 4 + (k & 3)] = g.v[t];
}

__device__ __forceinline__ int lit_ext(int lit) { return lit >= 15 ? 1 + (lit - 15) / 255 : 0; }

// inclusive scans over the 256 threads' values in LDS (Hillis-Steele); OP: 0 sum, 1 max, 2 min over the SUFFIX
template <int OP>
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t* buf, int tid) {
  buf[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < 256; d <<= 1) {
    uint32_t o;
    if (OP == 2) o = tid + d < 256 ? buf[tid + d] : kNone;
    else o = tid >= d ? buf[tid - d] : 0u;
    __syncthreads();
    if (OP == 0) v += o;
    else if (OP == 1) v = v > o ? v : o;
    else v = v < o ? v : o;
    buf[tid] = v;
    __syncthreads();
  }
  return v;
}

// byte e of the chunk (C order) from the strided source, 0 beyond the chunk's extent
__device__ __forceinline__ uint8_t chunk_byte(const DevChunksU8& a, unsigned e, const long long* o, const long long* x) {
  const unsigned cx = (unsigned)a.cx, cyx = (unsigned)a.cy * cx, czyx = (unsigned)a.cz * cyx;
  const unsigned c = e / czyx, r0 = e - c * czyx, z = r0 / cyx, r1 = r0 - z * cyx, y = r1 / cx, xx = r1 - y * cx;
  if ((long long)c < x[0] && (long long)z < x[1] && (long long)y < x[2] && (long long)xx < x[3])
    return a.src[(o[0] + c) * a.sc + (o[1] + z) * a.sz + (o[2] + y) * a.sy + (o[3] + xx)];
  return 0;
}

__global__ __launch_bounds__(256) void blosc_u8_block_kernel(const DevChunksU8 a, uint8_t* __restrict__ scratch, uint32_t* __restrict__ block_sizes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint8_t* s = lds + kOffS;
  uint16_t* A = (uint16_t*)(lds + kOffA);
  uint8_t* B = lds + kOffB;
  uint32_t* table = (uint32_t*)(lds + kOffT);
  uint32_t* buf = (uint32_t*)(lds + kOffBuf);
  uint32_t* entry = (uint32_t*)(lds + kOffEnt);
  const unsigned chunk = blockIdx.x / (unsigned)a.nblocks, blk = blockIdx.x % (unsigned)a.nblocks;
  const int tid = threadIdx.x;
  const unsigned e0 = blk * (unsigned)kBlock;
  const int n = (int)(a.chunk_bytes - e0 < (unsigned)kBlock ? a.chunk_bytes - e0 : (unsigned)kBlock);
  {
    long long o[4], x[4];
    for (int k = 0; k < 4; ++k) { o[k] = a.origin[4 * chunk + k]; x[k] = a.extent[4 * chunk + k]; }
    for (int j = tid; j < n; j += 256) s[j] = chunk_byte(a, e0 + (unsigned)j, o, x);
    if (tid < 16) s[n + tid] = 0;
  }
  for (int j = tid; j < (1 << kHashBits); j += 256) table[j] = 0;
  entry[tid] = kNone;
  __syncthreads();
  const int lo = tid * kSeg, hi = lo + kSeg < n ? lo + kSeg : n;   // (hi <= lo: the segment lies beyond the block)
  // ---- 0: run candidates.  A break is a position whose byte differs from the one before it (and position 0).
  {
    auto brk = [&](int i) { return i == 0 || s[i] != s[i - 1]; };
    uint32_t first = kNone;
    for (int i = lo; i < hi; ++i)
      if (brk(i)) { first = (uint32_t)i; break; }
    scan256<2>(first, buf, tid);
    uint32_t after = tid + 1 < 256 ? buf[tid + 1] : kNone;   // the first break behind the segment
    if (after == kNone) after = (uint32_t)n;
    __syncthreads();
    int nbk = (int)after;
    for (int i = hi - 1; i >= lo; --i) {
      if (brk(i)) nbk = i;
      const int cap = n - 5 - i;
      const int lr = nbk - i < cap ? nbk - i : cap;
      A[i] = (uint16_t)((i >= 1 && i <= n - 12 && lr >= kMinRun) ? (0x8000 | lr) : 0);
    }
  }
  __syncthreads();
  // ---- 1: table candidates and the choice, group by group
  {
    const uint32_t* sw = (const uint32_t*)s;
    const int ngroups = (n + 255) >> 8;
    for (int g = 0; g < ngroups; ++g) {
      const int i = g * 256 + tid;
      const bool has = i + 4 <= n;
      uint32_t h = 0;
      if (has) {
        const uint64_t w = (uint64_t)sw[i >> 2] | (uint64_t)sw[(i >> 2) + 1] << 32;
        h = ((uint32_t)(w >> (8 * (i & 3))) * 2654435761u) >> (32 - kHashBits);
        const uint32_t tv = table[h];
        if (tv && i <= n - 12) {
          const int c = (int)tv - 1;
          const int cap = n - 5 - i, lim = cap < kMaxTableLen ? cap : kMaxTableLen;
          const int lr = A[i] & 0x7fff;
          int lt = 0;
          if (lr < lim)   // (a run candidate of the table's cut or more wins whatever the comparison finds: inside long runs it is skipped)
            while (lt < lim && s[c + lt] == s[i + lt]) ++lt;
          if (lt >= kMinTable && lt > lr) { A[i] = (uint16_t)(i - c); B[i] = (uint8_t)lt; }
        }
      }
      __syncthreads();
      if (has) atomicMax(&table[h], (uint32_t)(i + 1));
      __syncthreads();
    }
  }
  // ---- 2: for every position of the segment, the last chain position inside the segment
  for (int i = hi - 1; i >= lo; --i) {
    const uint32_t av = A[i];
    const int tl = (av && !(av & 0x8000)) ? B[i] : 0;
    const int len = (av & 0x8000) ? (int)(av & 0x7fff) : tl;
    const int nx = i + (len ? len : 1);
    if (nx >= hi) B[i] = (uint8_t)(128 + tl);
    else { const uint8_t bn = B[nx]; B[i] = bn >= 128 ? (uint8_t)(nx - lo) : bn; }
  }
  __syncthreads();
  // ---- 3: the entries of the segments
  if (tid == 0) {
    int e = 0;
    while (e < n) {
      const int sg = e >> 7;
      entry[sg] = (uint32_t)e;
      const uint8_t bb = B[e];
      const int l = bb >= 128 ? e : (sg << 7) + bb;
      const uint32_t av = A[l];
      const int len = (av & 0x8000) ? (int)(av & 0x7fff) : (av ? (int)B[l] - 128 : 0);
      const int nx = l + (len > 0 ? len : 1);
      e = nx > e ? nx : e + 1;   // (always the former: the walk cannot stall whatever the arrays hold)
    }
  }
  __syncthreads();
  // ---- 4: the sequences.  First pass: the lengths of the visited table matches back into B (step 2 overwrote most of them).
  const int ent = entry[tid] == kNone ? hi : (int)entry[tid];
  uint32_t lle = 0;
  for (int i = ent; i < hi;) {
    const uint32_t av = A[i];
    if (!av) { ++i; continue; }
    int len;
    if (av & 0x8000) len = (int)(av & 0x7fff);
    else {
      const uint8_t bb = B[i];
      if (bb >= 128) len = bb - 128;
      else {
        const int c = i - (int)av, cap = n - 5 - i, lim = cap < kMaxTableLen ? cap : kMaxTableLen;
        len = 0;
        while (len < lim && s[c + len] == s[i + len]) ++len;
      }
      B[i] = (uint8_t)len;
    }
    i += len > 0 ? len : 1;
    lle = (uint32_t)i;
  }
  auto for_seqs = [&](auto&& f) {   // f(start, length, offset) for the sequences that START in this segment
    for (int i = ent; i < hi;) {
      const uint32_t av = A[i];
      if (!av) { ++i; continue; }
      const int len = (av & 0x8000) ? (int)(av & 0x7fff) : (int)B[i];
      f(i, len, (av & 0x8000) ? 1 : (int)av);
      i += len > 0 ? len : 1;
    }
  };
  scan256<1>(lle, buf, tid);
  const uint32_t before = tid ? buf[tid - 1] : 0u;   // the end of the last match before the segment
  const uint32_t q_last = buf[255];
  __syncthreads();
  uint32_t mine = 0;
  {
    int q = (int)before;
    for_seqs([&](int p, int L, int) {
      const int lit = p - q;
      mine += 1 + lit_ext(lit) + lit + 2 + lit_ext(L - 4);
      q = p + L;
    });
  }
  const uint32_t where = scan256<0>(mine, buf, tid) - mine;
  const uint32_t seq_total = buf[255];
  const int lit_f = n - (int)q_last;
  const uint32_t csize = seq_total + 1 + lit_ext(lit_f) + lit_f;
  const size_t slot_index = (size_t)chunk * (unsigned)a.nblocks + blk;
  uint8_t* slot = scratch + slot_index * kSlot;
  uint8_t* out = slot + 4;
  if (csize >= (uint32_t)n) {  // no gain: the block verbatim, marked by length == block size
    for (int j = tid; j < n / 4; j += 256) ((uint32_t*)out)[j] = ((const uint32_t*)s)[j];   // (slot + 4 is 4-byte aligned)
    if (tid < (n & 3)) out[(n & ~3) + tid] = s[(n & ~3) + tid];
    if (tid == 0) { *(uint32_t*)slot = (uint32_t)n; block_sizes[slot_index] = (uint32_t)n; }
    return;
  }
  auto put_len = [&](uint8_t*& o, int v) {                // the 255-steps of a length >= 15 (v = length - 15)
    for (; v >= 255; v -= 255) *o++ = 255;
    *o++ = (uint8_t)v;
  };
  {
    int q = (int)before;
    uint8_t* o = out + where;
    for_seqs([&](int p, int L, int off) {
      const int lit = p - q, m4 = L - 4;
      *o++ = (uint8_t)(((lit < 15 ? lit : 15) << 4) | (m4 < 15 ? m4 : 15));
      if (lit >= 15) put_len(o, lit - 15);
      for (int i = 0; i < lit; ++i) *o++ = s[q + i];
      *o++ = (uint8_t)(off & 255);
      *o++ = (uint8_t)(off >> 8);
      if (m4 >= 15) put_len(o, m4 - 15);
      q = p + L;
    });
  }
  // the closing literals: header by one thread, the bytes by all
  uint8_t* of = out + seq_total;
  const int hdr = 1 + lit_ext(lit_f);
  if (tid == 0) {
    uint8_t* o = of;
    *o++ = (uint8_t)((lit_f < 15 ? lit_f : 15) << 4);
    if (lit_f >= 15) put_len(o, lit_f - 15);
    *(uint32_t*)slot = csize;
    block_sizes[slot_index] = csize;
  }
  for (int i = tid; i < lit_f; i += 256) of[hdr + i] = s[q_last + i];
}

// Kernel 2, one workgroup per chunk: where every block goes (a prefix sum of the block sizes), header, block-start table.  A frame
// that would not be smaller than the chunk is stored (flag 2: header + the chunk's bytes), as c-blosc does.
__global__ __launch_bounds__(256) void blosc_u8_layout_kernel(const DevChunksU8 a, const uint32_t* __restrict__ block_sizes, uint32_t* __restrict__ starts,
                                                              uint8_t* __restrict__ frames, size_t slot_bytes, uint32_t* __restrict__ frame_sizes) {
  __shared__ uint32_t buf[256];
  const unsigned chunk = blockIdx.x;
  const int tid = threadIdx.x, nb = a.nblocks;
  uint8_t* f = frames + (size_t)chunk * slot_bytes;
  const uint32_t nbytes = a.chunk_bytes;
  const int per = (nb + 255) / 256, b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;   // (at most 4 blocks per thread)
  uint32_t mine = 0;
  for (int b = b0; b < b1; ++b) mine += 4 + block_sizes[(size_t)chunk * nb + b];
  uint32_t off = 16 + 4 * (uint32_t)nb + scan256<0>(mine, buf, tid) - mine;
  const uint32_t cbytes = 16 + 4 * (uint32_t)nb + buf[255];
  const bool stored = cbytes >= nbytes + 16;
  for (int b = b0; b < b1; ++b) {
    starts[(size_t)chunk * nb + b] = off;
    if (!stored)
      for (int j = 0; j < 4; ++j) f[16 + 4 * b + j] = (uint8_t)(off >> (8 * j));
    off += 4 + block_sizes[(size_t)chunk * nb + b];
  }
  if (tid == 0) {
    f[0] = 2; f[1] = 1; f[2] = (uint8_t)((stored ? 2 : 0) | 0x30); f[3] = 1;   // lz4 format, blocks not split
    const uint32_t w[3] = {nbytes, nbytes < (uint32_t)kBlock ? nbytes : (uint32_t)kBlock, stored ? nbytes + 16 : cbytes};
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 4; ++j) f[4 + 4 * k + j] = (uint8_t)(w[k] >> (8 * j));
    frame_sizes[chunk] = stored ? nbytes + 16 : cbytes;   // (nbytes + 16 exactly: only a stored frame has that size)
  }
}

// Kernel 3, one workgroup per (chunk, block): the block (its length prefix included) to its place in the frame, or, in a stored
// frame, the block's own bytes from the source.
__global__ __launch_bounds__(256) void blosc_u8_pack_kernel(const DevChunksU8 a, const uint8_t* __restrict__ scratch, const uint32_t* __restrict__ block_sizes,
                                                            const uint32_t* __restrict__ starts, uint8_t* __restrict__ frames, size_t slot_bytes,
                                                            const uint32_t* __restrict__ frame_sizes) {
  const unsigned chunk = blockIdx.x / (unsigned)a.nblocks, blk = blockIdx.x % (unsigned)a.nblocks;
  const int tid = threadIdx.x;
  uint8_t* f = frames + (size_t)chunk * slot_bytes;
  const size_t slot_index = (size_t)chunk * (unsigned)a.nblocks + blk;
  if (frame_sizes[chunk] == a.chunk_bytes + 16) {
    long long o[4], x[4];
    for (int k = 0; k < 4; ++k) { o[k] = a.origin[4 * chunk + k]; x[k] = a.extent[4 * chunk + k]; }
    const unsigned e0 = blk * (unsigned)kBlock;
    const unsigned n = a.chunk_bytes - e0 < (unsigned)kBlock ? a.chunk_bytes - e0 : (unsigned)kBlock;
    for (unsigned j = tid; j < n; j += 256) f[16 + (size_t)e0 + j] = chunk_byte(a, e0 + j, o, x);
    return;
  }
  const uint32_t off = starts[slot_index], len = 4 + block_sizes[slot_index];
  const uint8_t* src = scratch + slot_index * kSlot;
  for (uint32_t i = tid; i < len; i += 256) f[off + i] = src[i];
}

inline size_t blocks_of(size_t chunk_bytes) { return (chunk_bytes + kBlock - 1) / kBlock; }

}  // namespace
}  // namespace bsmi

using namespace bsmi;

extern "C" {

size_t bsmi_blosc_dev_u8_frame_bound(size_t chunk_bytes) { return chunk_bytes + 16 + 8 * blocks_of(chunk_bytes) + 64; }

size_t bsmi_blosc_dev_u8_scratch_bytes(int n_chunks, size_t chunk_bytes) {
  const size_t n = n_chunks > 0 ? (size_t)n_chunks : 0;
  return n * blocks_of(chunk_bytes) * ((size_t)kSlot + 8) + n * 8 * sizeof(long long) + 256;
}

int bsmi_blosc_encode_dev_u8(int device, const uint8_t* src_dev, const int64_t strides[3], int n_chunks, const int64_t* origins, const int64_t* extents,
                             const int64_t chunk_shape[4], void* scratch_dev, size_t scratch_bytes, void* frames_dev, size_t slot_bytes,
                             uint32_t* frame_sizes_dev, void* stream) {
  if (!src_dev || !strides || !origins || !extents || !chunk_shape || !scratch_dev || !frames_dev || !frame_sizes_dev || n_chunks < 1)
    BSMI_FAIL(BSMI_ERR_INVALID, "bsmi_blosc_encode_dev_u8: null argument");
  size_t chunk_bytes = 1;
  for (int d = 0; d < 4; ++d) {
    if (chunk_shape[d] < 1 || chunk_shape[d] > (int64_t)kMaxBlocks * kBlock) BSMI_FAIL(BSMI_ERR_INVALID, "device Blosc frames (1-byte items): bad chunk shape");
    chunk_bytes *= (size_t)chunk_shape[d];
    if (chunk_bytes > (size_t)kMaxBlocks * kBlock)
      BSMI_FAIL(BSMI_ERR_INVALID, "device Blosc frames (1-byte items) take chunks of at most %d blocks of 32 KiB: a larger chunk goes through the host codec", kMaxBlocks);
  }
  if (slot_bytes < bsmi_blosc_dev_u8_frame_bound(chunk_bytes) || scratch_bytes < bsmi_blosc_dev_u8_scratch_bytes(n_chunks, chunk_bytes))
    BSMI_FAIL(BSMI_ERR_INVALID, "device Blosc frames (1-byte items): scratch or frame slots too small");
  for (int i = 0; i < n_chunks; ++i)
    for (int d = 0; d < 4; ++d)
      if (origins[4 * i + d] < 0 || extents[4 * i + d] < 1 || extents[4 * i + d] > chunk_shape[d])
        BSMI_FAIL(BSMI_ERR_INVALID, "device Blosc frames (1-byte items): chunk %d has a bad extent", i);
  BSMI_HIP(hipSetDevice(device));
  static DeviceOnce once;
  if (int rc = once.run([&]() -> int {
        BSMI_HIP(hipFuncSetAttribute((const void*)blosc_u8_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
        return BSMI_OK;
      }))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)blocks_of(chunk_bytes);
  // scratch: [blocks][kSlot] | block sizes | block starts | origins, extents
  uint8_t* slots = (uint8_t*)scratch_dev;
  size_t off = (size_t)n_chunks * nb * kSlot;
  off = (off + 15) & ~(size_t)15;
  uint32_t* sizes = (uint32_t*)(slots + off);
  off += (size_t)n_chunks * nb * 4;
  off = (off + 15) & ~(size_t)15;
  uint32_t* starts = (uint32_t*)(slots + off);
  off += (size_t)n_chunks * nb * 4;
  off = (off + 15) & ~(size_t)15;
  long long* geo = (long long*)(slots + off);
  for (int first = 0; first < n_chunks; first += kGeoBatch) {
    GeoBatch g;
    const int count = n_chunks - first < kGeoBatch ? n_chunks - first : kGeoBatch;
    for (int i = 0; i < count; ++i)
      for (int d = 0; d < 4; ++d) {
        g.v[8 * i + d] = origins[4 * (first + i) + d];
        g.v[8 * i + 4 + d] = extents[4 * (first + i) + d];
      }
    for (int i = count * 8; i < kGeoBatch * 8; ++i) g.v[i] = 0;
    hipLaunchKernelGGL(geo_write_kernel, dim3(1), dim3(kGeoBatch * 8), 0, s, g, first, count, n_chunks, geo);
  }
  DevChunksU8 a;
  a.src = src_dev; a.sc = strides[0]; a.sz = strides[1]; a.sy = strides[2]; a.origin = geo; a.extent = geo + (size_t)n_chunks * 4;
  a.cc = (int)chunk_shape[0]; a.cz = (int)chunk_shape[1]; a.cy = (int)chunk_shape[2]; a.cx = (int)chunk_shape[3];
  a.chunk_bytes = (unsigned)chunk_bytes; a.nblocks = nb;
  hipLaunchKernelGGL(blosc_u8_block_kernel, dim3((unsigned)n_chunks * (unsigned)nb), dim3(256), kLds, s, a, slots, sizes);
  hipLaunchKernelGGL(blosc_u8_layout_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, a, (const uint32_t*)sizes, starts, (uint8_t*)frames_dev, slot_bytes,
                     frame_sizes_dev);
  hipLaunchKernelGGL(blosc_u8_pack_kernel, dim3((unsigned)n_chunks * (unsigned)nb), dim3(256), 0, s, a, (const uint8_t*)slots, (const uint32_t*)sizes,
                     (const uint32_t*)starts, (uint8_t*)frames_dev, slot_bytes, (const uint32_t*)frame_sizes_dev);
  BSMI_HIP(hipGetLastError());
  return BSMI_OK;
}

}  // extern "C"

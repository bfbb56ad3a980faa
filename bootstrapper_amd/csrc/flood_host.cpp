// The 3-D seeded watershed flood on the host.
//
// fragments_in_xy = false (reference post/ws.py:98-110) floods a whole block from ONE priority queue; skimage's heap order
// decides ties, so the loop is sequential by definition.  The device replay of it (seg_ws3.hip: ws3_flood_kernel) is one wave
// walking that loop at a global-memory round trip per pop: 12.8 s for a 128^3 block, where a host core takes 0.16 s
// (tools/probe_ws3.py).  So the device computes mask, distance transform, maxima and markers (the data-parallel part), this
// file floods, the device continues -- also in the block pipeline, whose 16 lanes made the device loop 0.8 s per block.
// bsmi_seg_set_host_flood(h, 0) selects the device loop (asynchronous; kept and tested).
//
// Algorithm: exactly ws3_flood_kernel's (and oracle/seg_ref.c's) -- entries ordered by (MAXD2 - d2, age) only; seeds pushed
// in raster order with age 0; heappush sifts up while strictly smaller than the parent, heappop moves the last entry to the
// root and sifts it down towards the smaller child; neighbours in the order [-HW, -W, -1, +1, +W, +HW], each unlabelled
// masked neighbour labelled and pushed with the next age.
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsmi {

// Entry: NARROW -- one 64-bit word (MAXD2 - d2) << 46 | age << 23 | voxel (what ws3_flood_kernel packs; volumes below 2^23
// voxels with D^2 + H^2 + W^2 + 2 D + 1 < 2^18), ordered by the bits above the voxel; otherwise WIDE -- the key
// (MAXD2 - d2) << 37 | age (d2 < 3 * 4096^2 + 2 * 4096 + 1 < 2^26, age < the voxel count <= 2^36) and the voxel beside it.
// Same order either way: (value, age), the voxel never compared.
struct FloodEntryNarrow {
  uint64_t e;
  static constexpr uint64_t MAXD2 = (1u << 18) - 1;
  FloodEntryNarrow(uint64_t d2, uint64_t age, size_t q) : e(((MAXD2 - d2) << 46) | (age << 23) | (uint64_t)q) {}
  bool operator<(const FloodEntryNarrow& o) const { return (e >> 23) < (o.e >> 23); }
  size_t voxel() const { return (size_t)(e & 0x7fffffu); }
};
struct FloodEntryWide {
  uint64_t key, q;
  static constexpr uint64_t MAXD2 = (1u << 26) - 1;
  FloodEntryWide(uint64_t d2, uint64_t age, size_t q_) : key(((MAXD2 - d2) << 37) | age), q((uint64_t)q_) {}
  bool operator<(const FloodEntryWide& o) const { return key < o.key; }
  size_t voxel() const { return (size_t)q; }
};

template <typename E>
static void flood3(int D, int H, int W, const uint8_t* mask, const int32_t* d2, int32_t* lab) {
  const size_t n = (size_t)D * H * W, hw = (size_t)H * W;
  std::vector<E> heap;
  heap.reserve(n / 4 + 1024);
  auto push = [&](const E it) {
    size_t c = heap.size();
    heap.push_back(it);
    while (c > 0) {
      const size_t p = (c + 1) / 2 - 1;
      const E pv = heap[p];
      if (it < pv) { heap[c] = pv; c = p; } else break;
    }
    heap[c] = it;
  };
  for (size_t j = 0; j < n; ++j)
    if (lab[j] != 0) push(E((uint64_t)d2[j], 0, j));
  uint64_t age = 0;
  while (!heap.empty()) {
    const E e = heap[0];
    const size_t items = heap.size() - 1;
    const size_t idx = e.voxel();
    const int32_t l = lab[idx];
    if (items > 0) {
      const E last = heap[items];
      size_t i = 0;
      for (;;) {
        const size_t c1 = 2 * i + 1, c2 = c1 + 1;
        if (c1 >= items) break;
        size_t sm = i;
        E smv = last;
        const E v1 = heap[c1];
        if (v1 < smv) { sm = c1; smv = v1; }
        if (c2 < items) {
          const E v2 = heap[c2];
          if (v2 < smv) { sm = c2; smv = v2; }
        }
        if (sm == i) break;
        heap[i] = smv;
        i = sm;
      }
      heap[i] = last;
    }
    heap.pop_back();
    const int x = (int)(idx % W), y = (int)((idx / W) % H), z = (int)(idx / hw);
    const bool ok[6] = {z > 0, y > 0, x > 0, x < W - 1, y < H - 1, z < D - 1};
    const long long dq[6] = {-(long long)hw, -(long long)W, -1, 1, (long long)W, (long long)hw};
    for (int k = 0; k < 6; ++k) {
      if (!ok[k]) continue;
      const size_t q = (size_t)((long long)idx + dq[k]);
      if (!mask[q] || lab[q] != 0) continue;
      ++age;
      lab[q] = l;
      push(E((uint64_t)d2[q], age, q));
    }
  }
}

void host_flood3(int D, int H, int W, const uint8_t* mask, const int32_t* d2, int32_t* lab) {
  const size_t n = (size_t)D * H * W;
  if (n < ((size_t)1 << 23) && (size_t)D * D + (size_t)H * H + (size_t)W * W + 2 * D + 1 < ((size_t)1 << 18))
    flood3<FloodEntryNarrow>(D, H, W, mask, d2, lab);
  else
    flood3<FloodEntryWide>(D, H, W, mask, d2, lab);
}

}  // namespace bsmi

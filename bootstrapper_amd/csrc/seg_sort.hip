// The radix sorts of the segmentation engine (node ids and sorted edge numbering of the RAG path, ids of the label table).
// The only file of the engine that includes hipcub: its rocPRIM kernels are instantiated here, once.
#include <hipcub/hipcub.hpp>

#include "seg_internal.h"

namespace bsmi {

hipError_t seg_sort_tmp_bytes(int n_keys, int n_pairs, size_t* bytes) {
  size_t b1 = 0, b2 = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, b1, (const uint64_t*)nullptr, (uint64_t*)nullptr, n_keys);
  if (e == hipSuccess)
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, b2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, n_pairs);
  *bytes = std::max(b1, b2);
  return e;
}

hipError_t seg_sort_keys_u64(void* tmp, size_t tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, int n, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys_in, keys_out, n, 0, 64, s);
}

hipError_t seg_sort_pairs_u64_u32(void* tmp, size_t tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* vals_in,
                                  uint32_t* vals_out, int n, hipStream_t s) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, 64, s);
}

}  // namespace bsmi

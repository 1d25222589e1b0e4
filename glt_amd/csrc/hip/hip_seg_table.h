/* The segment table of the multi-segment feature stores
 * (hip_unified_tensor.hip, hip_quant_feature.hip): a logical row space that
 * is the concatenation of up to kMaxSegs physical segments (HBM, xGMI peer
 * memory, host-mapped views), passed to the gather kernels by value so the
 * lookup runs on kernel arguments.
 */
#pragma once

#include <vector>

#include "hip_common.h"

namespace glt {

constexpr int kMaxSegs = 16;

struct SegTable {
  const char* base[kMaxSegs];
  int64_t row_start[kMaxSegs + 1];  // ascending; row r in seg s iff
                                    // row_start[s] <= r < row_start[s+1]
  int n;
};

// First byte of logical row r, rows row_bytes apart within a segment.
__device__ __forceinline__ const char* seg_row(const SegTable& segs,
                                               int64_t r,
                                               int64_t row_bytes) {
  int s = 0;
  while (s + 1 < segs.n && r >= segs.row_start[s + 1]) ++s;
  return segs.base[s] + (r - segs.row_start[s]) * row_bytes;
}

inline SegTable make_seg_table(const std::vector<torch::Tensor>& segs) {
  SegTable t;
  t.n = (int)segs.size();
  int64_t acc = 0;
  for (int i = 0; i < t.n; ++i) {
    t.base[i] = reinterpret_cast<const char*>(segs[i].data_ptr());
    t.row_start[i] = acc;
    acc += segs[i].size(0);
  }
  t.row_start[t.n] = acc;
  return t;
}

}  // namespace glt

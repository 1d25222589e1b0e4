/* Wave64 lane helpers shared by the attention kernels (hip_gat.hip,
 * hip_gatv2.hip): one wave per row of up to 128 channels, two per lane.
 */
#pragma once

#include <type_traits>

#include "hip_common.h"

namespace glt {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int sft = kWave / 2; sft > 0; sft >>= 1) v += __shfl_down(v, sft);
  return __shfl(v, 0);
}

// A lane's two channels of a [C] row.  kPair (C even, rows aligned to two
// elements): channels 2*lane and 2*lane + 1 in one 4-byte (bf16) or 8-byte
// (fp32) load, C <= 128 in one pass.  Otherwise channels lane and
// 64 + lane, two scalar loads.  Lanes past the row read 0 and store nothing.
template <typename T, bool kPair>
__device__ __forceinline__ void row_load(const T* __restrict__ row, int lane,
                                         int C, float& a, float& b) {
  if constexpr (kPair) {
    a = 0.f;
    b = 0.f;
    if (2 * lane < C) {
      if constexpr (std::is_same<T, float>::value) {
        const float2 w = *reinterpret_cast<const float2*>(row + 2 * lane);
        a = w.x;
        b = w.y;
      } else {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(row + 2 * lane);
        a = __uint_as_float(w << 16);
        b = __uint_as_float(w & 0xffff0000u);
      }
    }
  } else {
    a = lane < C ? (float)row[lane] : 0.f;
    b = kWave + lane < C ? (float)row[kWave + lane] : 0.f;
  }
}

template <typename T, bool kPair>
__device__ __forceinline__ void row_store(T* __restrict__ row, int lane,
                                          int C, float a, float b) {
  if constexpr (kPair) {
    if (2 * lane < C) {
      if constexpr (std::is_same<T, float>::value) {
        *reinterpret_cast<float2*>(row + 2 * lane) = make_float2(a, b);
      } else {
        // c10's float -> bf16: RNE, as Tensor.to()
        *reinterpret_cast<uint32_t*>(row + 2 * lane) =
            (uint32_t)c10::BFloat16(a).x |
            ((uint32_t)c10::BFloat16(b).x << 16);
      }
    }
  } else {
    if (lane < C) row[lane] = (T)a;
    if (kWave + lane < C) row[kWave + lane] = (T)b;
  }
}

}  // namespace glt

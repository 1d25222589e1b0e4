/* Wave64 lane helpers shared by the attention kernels (hip_gat.hip,
 * hip_gatv2.hip): one wave per row of up to 128 channels, two per lane; and
 * by hip_tconv.hip: four channels per lane, heads as groups of lanes.
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

// ---------------------------------------------------------------------------
// Helpers that call nothing from the runtime headers (no __shfl*, no c10
// constructors), so that a file which switches the packed-fp32 target
// feature off for its device code (hip_tconv.hip) can include this header
// inside its pragma and have them inlined: a function declared under other
// features that is not forced inline would stay a call.
// ---------------------------------------------------------------------------

// v of lane (lane ^ mask)
__device__ __forceinline__ float lane_xor(float v, int lane, int mask) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2,
                                          __builtin_bit_cast(int, v)));
}

// Sums over aligned groups of G adjacent lanes (G a power of two <= 64), NV
// independent chains interleaved.  An xor butterfly: both partners of a
// level add the same two numbers, so every lane of a group ends with the
// same bits and no broadcast follows.
template <int NV>
__device__ __forceinline__ void group_sum(float (&x)[NV], int lane, int G) {
  for (int mask = 1; mask < G; mask <<= 1) {
    float o[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) o[j] = lane_xor(x[j], lane, mask);
#pragma unroll
    for (int j = 0; j < NV; ++j) x[j] += o[j];
  }
}

// float -> bf16 bits, round to nearest even (what Tensor.to() does)
__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <typename T>
__device__ __forceinline__ float elem_load(const T* p) {
  if constexpr (std::is_same<T, float>::value) {
    return *p;
  } else {
    return __builtin_bit_cast(
        float, (uint32_t) * reinterpret_cast<const uint16_t*>(p) << 16);
  }
}

template <typename T>
__device__ __forceinline__ void elem_store(T* p, float a) {
  if constexpr (std::is_same<T, float>::value) {
    *p = a;
  } else {
    *reinterpret_cast<uint16_t*>(p) = (uint16_t)bf16_rne(a);
  }
}

// Four consecutive channels in one load or store: 16 bytes (fp32) or 8
// (bf16); p is aligned to four elements.
template <typename T>
__device__ __forceinline__ void quad_load(const T* p, float (&v)[4]) {
  if constexpr (std::is_same<T, float>::value) {
    const float4 w = *reinterpret_cast<const float4*>(p);
    v[0] = w.x;
    v[1] = w.y;
    v[2] = w.z;
    v[3] = w.w;
  } else {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    v[0] = __builtin_bit_cast(float, w.x << 16);
    v[1] = __builtin_bit_cast(float, w.x & 0xffff0000u);
    v[2] = __builtin_bit_cast(float, w.y << 16);
    v[3] = __builtin_bit_cast(float, w.y & 0xffff0000u);
  }
}

template <typename T>
__device__ __forceinline__ void quad_store(T* p, const float (&v)[4]) {
  if constexpr (std::is_same<T, float>::value) {
    float4 w;
    w.x = v[0];
    w.y = v[1];
    w.z = v[2];
    w.w = v[3];
    *reinterpret_cast<float4*>(p) = w;
  } else {
    uint2 w;
    w.x = bf16_rne(v[0]) | (bf16_rne(v[1]) << 16);
    w.y = bf16_rne(v[2]) | (bf16_rne(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = w;
  }
}

// A lane's share of an item of n channels starting at p.  kQuad: channels
// 4*lane .. 4*lane + 3 (n % 4 == 0, p aligned to four elements, n <= 256).
// Otherwise channels lane and 64 + lane by scalar accesses (n <= 128), and
// v[2], v[3] are 0.  Lanes past the item read 0 and store nothing.
template <typename T, bool kQuad>
__device__ __forceinline__ void item_load(const T* p, int lane, int n,
                                          float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if constexpr (kQuad) {
    if (4 * lane < n) quad_load<T>(p + 4 * lane, v);
  } else {
    if (lane < n) v[0] = elem_load<T>(p + lane);
    if (kWave + lane < n) v[1] = elem_load<T>(p + kWave + lane);
  }
}

template <typename T, bool kQuad>
__device__ __forceinline__ void item_store(T* p, int lane, int n,
                                           const float (&v)[4]) {
  if constexpr (kQuad) {
    if (4 * lane < n) quad_store<T>(p + 4 * lane, v);
  } else {
    if (lane < n) elem_store<T>(p + lane, v[0]);
    if (kWave + lane < n) elem_store<T>(p + kWave + lane, v[1]);
  }
}

}  // namespace glt

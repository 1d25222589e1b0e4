/* Fused segment-mean aggregation for GNN convs (gfx950).
 *
 * The glt_amd sampler emits batch edges sorted by target local id, so the
 * per-target segments are contiguous: forward is one wave-per-target kernel
 * (no atomics, fused mean).  Backward, two forms: the gather backward
 * (seg_mean_bwd_gather_kernel, the python layer's default) sums dY/deg per
 * source row through an inverted index of the edges, without atomics or
 * an arena; the scatter backward (seg_mean_bwd_kernel) adds dY/deg into
 * an fp32 arena with atomics (same contention class as torch index_add_,
 * but fused with the degree division and vectorized).
 *
 * Scatter backward: plain fp32 atomics, so low-order bits depend on the
 * order in which they land.  order_independent = true (the python layer
 * passes it in deterministic mode, see glt_amd/ops/segment.py) trades
 * precision for run-to-run reproducibility: every contribution is first
 * snapped to a common power-of-two grid q = 2^(e + kGridHeadroomBits - 24),
 * 2^e > max|dY| (absmax pre-pass fused into the arena's zero fill), so
 * each fp32 partial sum below 2^24 q = 2^kGridHeadroomBits * 2^e is exact
 * and addition order cannot matter.  A dX element that collects more than
 * that (>= 64x the largest |dY|) rounds like ordinary fp32 again and loses
 * the guarantee.  Snapping costs up to q/2 <= 2^-18 max|dY| ABSOLUTE per
 * term: terms far below max|dY| lose relative precision or vanish, which
 * is why it is not the default.
 *
 * Replaces the 4-kernel torch sequence (bincount + index_select +
 * index_add_ + div) in SAGEConv (glt_amd/models/layers.py).
 *
 * dtype: templated over fp32 and bf16 inputs with fp32 accumulation —
 * the kernels are HBM-bound (see profiles/), so bf16 halves the roofline
 * traffic.  The scatter backward always accumulates into an fp32 arena
 * (bf16 atomics lose too much precision for degree-weighted sums) and the
 * python wrapper casts once at the end; the gather backward sums in fp32
 * registers and stores dy's dtype itself.
 *
 * seg_wsum_*: the weighted segment sum behind GCNConv and edge weights
 * (out[t] = a[t] * sum_e w[e] * b[col[e]] * x[col[e]]) with its dx and
 * per-edge dw backward; same layout, arena and order-independent mode.
 *
 * seg_ext_*: segment max / min with the arg of the first winning edge
 * (SAGEConv aggr='max' / 'min'); forward in the seg_wsum layout, backward
 * one atomic per output element into the same arena.
 */
#include <hip/hip_bf16.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "hip_common.h"
#include "../include/common.h"

namespace glt {

namespace {

// out[t, :F] = mean_{e in [off[t], off[t+1])} x[col[e], :]
// One wave per target row; lanes cover the feature dim.
// kCat: out is [n_tgt, 2F] and out[t, F:] = x[t, :], the fused
// [mean-agg | x_root] assembly.  Saves the dim-1 torch.cat (two copyBuffer
// passes over [n, F] per layer, ~260 us/step in the flagship profile) and
// its launches; valid for the homo SAGE path where targets are the row
// prefix of x (the sampler's local-id invariant).
template <typename scalar_t, bool kCat>
__global__ void seg_mean_fwd_kernel(const scalar_t* __restrict__ x,
                                    const int64_t* __restrict__ col,
                                    const int64_t* __restrict__ off,
                                    int64_t n_tgt, int64_t feat,
                                    scalar_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * feat : feat;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    const float inv = e > s ? 1.0f / (float)(e - s) : 0.0f;
    if (feat <= 2 * kWave) {
      // lane owns channels f and f+64: register accumulators + row
      // addresses batched 8 deep (independent gather misses)
      const int64_t f0 = lane, f1 = lane + kWave;
      float a0 = 0.f, a1 = 0.f;
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        int64_t cc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
          cc[q] = (q < nb ? col[k0 + q] : col[k0]) * feat;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (q < nb) {
            if (f0 < feat) a0 += static_cast<float>(x[cc[q] + f0]);
            if (f1 < feat) a1 += static_cast<float>(x[cc[q] + f1]);
          }
        }
      }
      if (f0 < feat) {
        out[t * ostride + f0] = static_cast<scalar_t>(a0 * inv);
        if constexpr (kCat) out[t * ostride + feat + f0] = x[t * feat + f0];
      }
      if (f1 < feat) {
        out[t * ostride + f1] = static_cast<scalar_t>(a1 * inv);
        if constexpr (kCat) out[t * ostride + feat + f1] = x[t * feat + f1];
      }
      continue;
    }
    for (int64_t f = lane; f < feat; f += kWave) {
      float acc = 0.f;
      for (int64_t k = s; k < e; ++k)
        acc += static_cast<float>(x[col[k] * feat + f]);
      out[t * ostride + f] = static_cast<scalar_t>(acc * inv);
      if constexpr (kCat) out[t * ostride + feat + f] = x[t * feat + f];
    }
  }
}

// bf16 fast path: each lane owns TWO adjacent channels (one 4-byte
// ushort2 load per row visit) — the scalar template's 2-byte gathers
// were measured at only 1.36x fp32 on the HBM-bound forward.
template <bool kCat>
__global__ void seg_mean_fwd_bf162_kernel(const __hip_bfloat162* __restrict__ x,
                                          const int64_t* __restrict__ col,
                                          const int64_t* __restrict__ off,
                                          int64_t n_tgt, int64_t feat2,
                                          __hip_bfloat162* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * feat2 : feat2;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    const float inv = e > s ? 1.0f / (float)(e - s) : 0.0f;
    if (feat2 <= kWave) {
      // one channel-pair per lane: accumulate in registers with the
      // row addresses batched 8 deep, so the gather issues 8
      // independent misses instead of a serial col->row->col chain
      const int64_t f = lane;
      const bool act = f < feat2;
      float2 acc = {0.f, 0.f};
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        int64_t cc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q)
          cc[q] = (q < nb ? col[k0 + q] : col[k0]) * feat2;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          if (q < nb && act) {
            const float2 v = __bfloat1622float2(x[cc[q] + f]);
            acc.x += v.x;
            acc.y += v.y;
          }
        }
      }
      if (act) {
        out[t * ostride + f] =
            __float22bfloat162_rn({acc.x * inv, acc.y * inv});
        if constexpr (kCat) out[t * ostride + feat2 + f] = x[t * feat2 + f];
      }
      continue;
    }
    for (int64_t f = lane; f < feat2; f += kWave) {
      float2 acc = {0.f, 0.f};
      for (int64_t k = s; k < e; ++k) {
        const float2 v = __bfloat1622float2(x[col[k] * feat2 + f]);
        acc.x += v.x;
        acc.y += v.y;
      }
      out[t * ostride + f] =
          __float22bfloat162_rn({acc.x * inv, acc.y * inv});
      if constexpr (kCat) out[t * ostride + feat2 + f] = x[t * feat2 + f];
    }
  }
}

constexpr int kGridHeadroomBits = 6;

// few, fat blocks: every backward wave folds all the parts before it starts
constexpr int kMaxAmaxParts = 256;
constexpr int kZeroBlock = 1024;

// One launch in place of the arena's zero fill: zeroes arena[0, n_arena)
// and leaves max |x| over this block's grid-stride share of x in
// parts[blockIdx.x] (plain store; NaNs are skipped).  The backward
// kernel folds the gridDim.x parts itself, so the absmax pre-pass costs
// no launch of its own.
template <typename scalar_t>
__global__ void __launch_bounds__(kZeroBlock)
zero_absmax_kernel(float* __restrict__ arena, int64_t n_arena,
                   const scalar_t* __restrict__ x, int64_t n,
                   float* __restrict__ parts) {
  __shared__ float wm[kZeroBlock / kWave];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  // allocator blocks are >= 16 B aligned and the arena starts one
  const int64_t n4 = n_arena / 4;
  float4* a4 = reinterpret_cast<float4*>(arena);
  for (int64_t i = g0; i < n4; i += stride)
    a4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = n4 * 4 + g0; i < n_arena; i += stride) arena[i] = 0.f;
  float m = 0.f;
  for (int64_t i = g0; i < n; i += stride)
    m = fmaxf(m, fabsf(static_cast<float>(x[i])));
  for (int o = kWave / 2; o > 0; o >>= 1)
    m = fmaxf(m, __shfl_xor(m, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) wm[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kZeroBlock / kWave; ++w) m = fmaxf(m, wm[w]);
    parts[blockIdx.x] = m;
  }
}

// Magic constant 1.5 * 2^(e + kGridHeadroomBits - 1): (v + M) - M rounds
// |v| <= max|dY| < 2^e to a multiple of ulp(M) = q.  0 = do not snap
// (n_parts == 0: plain mode; empty / non-finite dY; q outside the normal
// range).  Wave-uniform: every lane folds the same n_parts <=
// kMaxAmaxParts block maxima.  scale (optional, one device float) is a
// bound on the factor each dY value is multiplied by before it is
// snapped: the grid then sits below max|dY| * scale, the largest term.
__device__ __forceinline__ float grid_magic(const float* __restrict__ parts,
                                            int n_parts,
                                            const float* __restrict__ scale =
                                                nullptr) {
  float a = 0.f;
  for (int i = threadIdx.x & (kWave - 1); i < n_parts; i += kWave)
    a = fmaxf(a, parts[i]);
  for (int o = kWave / 2; o > 0; o >>= 1)
    a = fmaxf(a, __shfl_xor(a, o, kWave));
  if (scale != nullptr) a *= fabsf(*scale);
  if (!(a > 0.f) || !isfinite(a)) return 0.f;
  int e;
  frexpf(a, &e);
  const int me = e + kGridHeadroomBits - 1;
  if (me > 120 || me < -100) return 0.f;
  return ldexpf(1.5f, me);
}

__device__ __forceinline__ float snap(float v, float magic) {
  return magic == 0.f ? v : __fsub_rn(__fadd_rn(v, magic), magic);
}

// dx[col[e], :] += dy[t, :F] / deg(t)  (dx is always fp32)
// kCat: dy is [n_tgt, 2F] and dx[t, :] += dy[t, F:] as well
template <typename scalar_t, bool kCat>
__global__ void seg_mean_bwd_kernel(const scalar_t* __restrict__ dy,
                                    const int64_t* __restrict__ col,
                                    const int64_t* __restrict__ off,
                                    int64_t n_tgt, int64_t feat,
                                    const float* __restrict__ amax_parts,
                                    int n_parts,
                                    float* __restrict__ dx) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * feat : feat;
  const float magic = grid_magic(amax_parts, n_parts);
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    if constexpr (kCat) {
      for (int64_t f = lane; f < feat; f += kWave)
        atomicAdd(&dx[t * feat + f],
                  snap(static_cast<float>(dy[t * ostride + feat + f]), magic));
    }
    if (e <= s) continue;
    const float inv = 1.0f / (float)(e - s);
    for (int64_t k = s; k < e; ++k) {
      const int64_t c = col[k];
      for (int64_t f = lane; f < feat; f += kWave)
        atomicAdd(&dx[c * feat + f],
                  snap(static_cast<float>(dy[t * ostride + f]) * inv, magic));
    }
  }
}

// The wave index is the same in all 64 lanes, but derived from
// threadIdx the compiler cannot see it: passing it through readfirstlane
// lets everything indexed by the target or the edge (offsets, col, and
// the w / a / b factors) use the scalar unit, one load per wave.
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi =
      __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---------------------------------------------------------------------------
// Atomic-free segment-mean backward: gather by source.
//   dx[s, :] = sum over in-edges (t -> s) of dy[t, :F] / deg(t)
//              (+ dy[s, F:] if s < n_tgt with kCat)
// summed in fp32 per SOURCE row through the inverted index of col
// (src_off / in_tgt, built by hip_segment_transpose), rounded once to dy's
// dtype and, with kMask, masked by the ReLU of the layer below.  One pass:
// no arena, no zero fill, no atomics, no separate cast or mask kernel.
// Every row of dx is stored, also rows nothing contributes to (zeros).
//
// The terms, inv, snap and grid_magic are those of seg_mean_bwd_kernel.  In
// order-independent mode, within the headroom, the fp32 sums are exact in
// any order, so the result has the bits of the atomic path followed by
// Tensor.to(dtype) and threshold_backward.  Each in-list keeps the edge
// order (stable sort), so plain mode is run-to-run identical too, which
// the atomic path is not.
//
// Known limit: one wave sums a source's whole in-list; a hub source with
// thousands of in-edges serialises on it (list splitting is the follow-up).
// ---------------------------------------------------------------------------

// src_off[k] = first position i of the sorted keys with key[i] >= k (and
// n_edge past the last key): position i fills k in (key[i-1], key[i]], the
// head [0, key[0]] and the tail (key[E-1], n_src] are spread over the grid.
// No atomics, no cumsum.  Keys outside [0, n_src) break the caller's
// contract; they are clamped so that no store leaves src_off.
__global__ void seg_boundary_kernel(const int64_t* __restrict__ key,
                                    int64_t n_edge, int64_t n_src,
                                    int64_t* __restrict__ src_off) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  auto clamped = [n_src](int64_t k) {
    return k < 0 ? (int64_t)-1 : (k < n_src ? k : n_src - 1);
  };
  const int64_t first = clamped(key[0]), last = clamped(key[n_edge - 1]);
  for (int64_t k = g0; k <= first; k += stride) src_off[k] = 0;
  for (int64_t k = last + 1 + g0; k <= n_src; k += stride)
    src_off[k] = n_edge;
  for (int64_t i = 1 + g0; i < n_edge; i += stride) {
    const int64_t hi = clamped(key[i]);
    for (int64_t k = clamped(key[i - 1]) + 1; k <= hi; ++k) src_off[k] = i;
  }
}

// A lane's share of one row per pass, as kVals fp32 channels.  Lanes past
// the row end read the row's last unit and do not store.
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  // c10's float -> bf16: RNE, as Tensor.to()
  return (uint32_t)c10::BFloat16(lo).x | ((uint32_t)c10::BFloat16(hi).x << 16);
}

// bf16, F % 4 == 0: rows are arrays of U = F / 4 units of four channels,
// one 8-byte load per lane per row visit, 256 channels per pass (a
// flagship row, F = 256, is one wave instruction).
struct GatherBf164 {
  using unit_t = uint2;
  static constexpr int kVals = 4;
  static constexpr int kUnitsPerPass = kWave;
  __device__ static __forceinline__ void load(const unit_t* __restrict__ p,
                                              int64_t row, int64_t fb,
                                              int lane, int64_t U,
                                              float (&v)[kVals]) {
    const int64_t u = fb + lane;
    const uint2 w = p[row + (u < U ? u : U - 1)];
    v[0] = __uint_as_float(w.x << 16);
    v[1] = __uint_as_float(w.x & 0xffff0000u);
    v[2] = __uint_as_float(w.y << 16);
    v[3] = __uint_as_float(w.y & 0xffff0000u);
  }
  __device__ static __forceinline__ void store(unit_t* __restrict__ p,
                                               int64_t row, int64_t fb,
                                               int lane, int64_t U,
                                               const float (&v)[kVals]) {
    const int64_t u = fb + lane;
    if (u < U) p[row + u] = make_uint2(pack_bf16(v[0], v[1]),
                                       pack_bf16(v[2], v[3]));
  }
};

// bf16, other even F: U = F / 2 channel pairs, one 4-byte load per lane
// per row visit, 128 channels per pass.
struct GatherBf162 {
  using unit_t = uint32_t;
  static constexpr int kVals = 2;
  static constexpr int kUnitsPerPass = kWave;
  __device__ static __forceinline__ void load(const unit_t* __restrict__ p,
                                              int64_t row, int64_t fb,
                                              int lane, int64_t U,
                                              float (&v)[kVals]) {
    const int64_t u = fb + lane;
    const uint32_t w = p[row + (u < U ? u : U - 1)];
    v[0] = __uint_as_float(w << 16);
    v[1] = __uint_as_float(w & 0xffff0000u);
  }
  __device__ static __forceinline__ void store(unit_t* __restrict__ p,
                                               int64_t row, int64_t fb,
                                               int lane, int64_t U,
                                               const float (&v)[kVals]) {
    const int64_t u = fb + lane;
    if (u < U) p[row + u] = pack_bf16(v[0], v[1]);
  }
};

// fp32, F % 4 == 0: U = F / 4 float4 units, 16 bytes per lane, 256
// channels per pass.
struct GatherF324 {
  using unit_t = float4;
  static constexpr int kVals = 4;
  static constexpr int kUnitsPerPass = kWave;
  __device__ static __forceinline__ void load(const unit_t* __restrict__ p,
                                              int64_t row, int64_t fb,
                                              int lane, int64_t U,
                                              float (&v)[kVals]) {
    const int64_t u = fb + lane;
    const float4 w = p[row + (u < U ? u : U - 1)];
    v[0] = w.x;
    v[1] = w.y;
    v[2] = w.z;
    v[3] = w.w;
  }
  __device__ static __forceinline__ void store(unit_t* __restrict__ p,
                                               int64_t row, int64_t fb,
                                               int lane, int64_t U,
                                               const float (&v)[kVals]) {
    const int64_t u = fb + lane;
    if (u < U) p[row + u] = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// Any other fp32 F, and bf16 with odd F: U = F channels, a lane owns f and
// f + 64 (128 channels per pass).
template <typename scalar_t>
struct GatherScalar {
  using unit_t = scalar_t;
  static constexpr int kVals = 2;
  static constexpr int kUnitsPerPass = 2 * kWave;
  __device__ static __forceinline__ void load(const unit_t* __restrict__ p,
                                              int64_t row, int64_t fb,
                                              int lane, int64_t U,
                                              float (&v)[kVals]) {
    const int64_t u0 = fb + lane, u1 = fb + lane + kWave;
    v[0] = static_cast<float>(p[row + (u0 < U ? u0 : U - 1)]);
    v[1] = fb + kWave < U  // wave-uniform
               ? static_cast<float>(p[row + (u1 < U ? u1 : U - 1)])
               : 0.f;
  }
  __device__ static __forceinline__ void store(unit_t* __restrict__ p,
                                               int64_t row, int64_t fb,
                                               int lane, int64_t U,
                                               const float (&v)[kVals]) {
    const int64_t u0 = fb + lane, u1 = fb + lane + kWave;
    if (u0 < U) p[row + u0] = static_cast<scalar_t>(v[0]);
    if (u1 < U) p[row + u1] = static_cast<scalar_t>(v[1]);
  }
};

// Target row and 1 / deg of the in-list entry at position k, in scalar
// registers.  in_tgt holds the TARGET id of each in-edge (not its edge
// position: that would cost a search of off per edge).  An entry that
// names no target of this call (t outside [0, n_tgt)) contributes nothing,
// like an edge past off[n_tgt] on the atomic path.
__device__ __forceinline__ void gather_entry(const int64_t* __restrict__ in_tgt,
                                             const int64_t* __restrict__ off,
                                             int64_t k, int64_t n_tgt,
                                             int64_t ostride, int64_t& row,
                                             float& inv, bool& use) {
  int64_t t = in_tgt[k];
  use = t >= 0 && t < n_tgt;
  if (!use) t = 0;
  const int64_t deg = off[t + 1] - off[t];
  inv = 1.0f / (float)deg;
  row = t * ostride;
}

// List bounds of kRows consecutive sources and the first entry of each
// list: everything a wave needs before it can issue a block's row loads,
// all in scalar registers (three dependent scalar loads).
template <int kRows>
struct GatherBlock {
  int64_t lb[kRows + 1];
  int64_t row0[kRows];
  float inv0[kRows];
  bool use0[kRows];

  __device__ __forceinline__ void load(const int64_t* __restrict__ src_off,
                                       const int64_t* __restrict__ in_tgt,
                                       const int64_t* __restrict__ off,
                                       int64_t s0, int64_t n_src,
                                       int64_t n_tgt, int64_t ostride) {
    // rows past n_src get an empty list (both bounds src_off[n_src])
#pragma unroll
    for (int r = 0; r <= kRows; ++r)
      lb[r] = src_off[s0 + r < n_src ? s0 + r : n_src];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      row0[r] = 0;
      inv0[r] = 0.f;
      use0[r] = false;
      if (lb[r + 1] > lb[r])
        gather_entry(in_tgt, off, lb[r], n_tgt, ostride, row0[r], inv0[r],
                     use0[r]);
    }
  }
};

// The mean in-degree of a sampled batch is about 1.1, so there is nothing
// to batch along a list.  A wave takes kRows consecutive sources, whose
// list bounds, first in-edges and dy / root / mask row loads are issued
// together, and while those row loads are in flight it runs the scalar
// loads of its NEXT block, so the two dependent chains overlap.  Longer
// lists continue in an inner loop, four entries per batch, added in list
// order.
template <typename P, bool kCat, bool kMask, int kRows>
__global__ void seg_mean_bwd_gather_kernel(
    const typename P::unit_t* __restrict__ dy, const int64_t* __restrict__ off,
    const int64_t* __restrict__ src_off, const int64_t* __restrict__ in_tgt,
    const typename P::unit_t* __restrict__ mask, int64_t n_tgt, int64_t n_src,
    int64_t U, const float* __restrict__ amax_parts, int n_parts,
    typename P::unit_t* __restrict__ out) {
  constexpr int kVals = P::kVals;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * U : U;
  const int64_t n_blk = (n_src + kRows - 1) / kRows;
  GatherBlock<kRows> cur = {}, nxt = {};
  if (wave < n_blk)
    cur.load(src_off, in_tgt, off, wave * kRows, n_src, n_tgt, ostride);
  const float magic = grid_magic(amax_parts, n_parts);
  for (int64_t blk = wave; blk < n_blk; blk += n_waves) {
    const int64_t s0 = blk * kRows;
    for (int64_t fb = 0; fb < U; fb += P::kUnitsPerPass) {
      float root[kRows][kVals], m[kRows][kVals], v[kRows][kVals];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int64_t s = s0 + r;
#pragma unroll
        for (int j = 0; j < kVals; ++j) root[r][j] = m[r][j] = 0.f;
        if (kCat && s < n_tgt)
          P::load(dy, s * ostride + U, fb, lane, U, root[r]);
        if (kMask && s < n_src) P::load(mask, s * U, fb, lane, U, m[r]);
        P::load(dy, cur.row0[r], fb, lane, U, v[r]);
      }
      if (fb == 0 && blk + n_waves < n_blk)
        nxt.load(src_off, in_tgt, off, (blk + n_waves) * kRows, n_src, n_tgt,
                 ostride);
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int64_t s = s0 + r;
        if (s >= n_src) break;
        float acc[kVals];
#pragma unroll
        for (int j = 0; j < kVals; ++j) {
          acc[j] = 0.f;
          if (kCat && s < n_tgt) acc[j] += snap(root[r][j], magic);
          if (cur.use0[r]) acc[j] += snap(v[r][j] * cur.inv0[r], magic);
        }
        for (int64_t k0 = cur.lb[r] + 1; k0 < cur.lb[r + 1]; k0 += 4) {
          const int nb =
              (int)((cur.lb[r + 1] - k0) < 4 ? (cur.lb[r + 1] - k0) : 4);
          int64_t row[4];
          float inv[4];
          bool use[4];
          float w[4][kVals];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            gather_entry(in_tgt, off, q < nb ? k0 + q : k0, n_tgt, ostride,
                         row[q], inv[q], use[q]);
#pragma unroll
          for (int q = 0; q < 4; ++q) P::load(dy, row[q], fb, lane, U, w[q]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q < nb && use[q]) {  // wave-uniform
#pragma unroll
              for (int j = 0; j < kVals; ++j)
                acc[j] += snap(w[q][j] * inv[q], magic);
            }
          }
        }
        // threshold_backward's rule: a NaN mask passes, masked gives +0
#pragma unroll
        for (int j = 0; j < kVals; ++j)
          if (kMask && m[r][j] <= 0.f) acc[j] = 0.f;
        P::store(out, s * U, fb, lane, U, acc);
      }
    }
    cur = nxt;
  }
}

// ---------------------------------------------------------------------------
// Weighted segment sum (GCN-style aggregation):
//   out[t, :] = a[t] * sum_{e in [off[t], off[t+1])} w[e] * b[col[e]] * x[col[e], :]
// w (per edge), a (per target) and b (per source) are optional fp32
// factors; a null pointer means 1.  The per-edge coefficient w[e] * b[c]
// has a wave-uniform address, so it is loaded once per edge and not once
// per lane-channel.  Same wave-per-target layout as seg_mean_fwd_kernel.
// ---------------------------------------------------------------------------

// Row addresses and factors of up to 8 edges starting at k0, all in
// scalar registers.  Slots past the end of the segment repeat edge k0 (a
// valid row) so the loads that follow need no branch; the caller drops
// their products.  A null w or b means 1.
__device__ __forceinline__ void wsum_edge_batch(
    const int64_t* __restrict__ col, const float* __restrict__ w,
    const float* __restrict__ b, int64_t k0, int nb, int64_t stride,
    int64_t (&cc)[8], float (&cw)[8], float (&cb)[8]) {
  int64_t c[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) c[q] = col[q < nb ? k0 + q : k0];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    cc[q] = c[q] * stride;
    cw[q] = 1.0f;
    cb[q] = 1.0f;
  }
  if (w != nullptr) {
#pragma unroll
    for (int q = 0; q < 8; ++q) cw[q] = w[q < nb ? k0 + q : k0];
  }
  if (b != nullptr) {
#pragma unroll
    for (int q = 0; q < 8; ++q) cb[q] = b[c[q]];
  }
}

template <typename scalar_t, bool kW, bool kB>
__global__ void seg_wsum_fwd_kernel(const scalar_t* __restrict__ x,
                                    const int64_t* __restrict__ col,
                                    const int64_t* __restrict__ off,
                                    const float* __restrict__ w,
                                    const float* __restrict__ a,
                                    const float* __restrict__ b,
                                    int64_t n_tgt, int64_t feat,
                                    scalar_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    const float at = a != nullptr ? a[t] : 1.0f;
    // 128 channels per pass (lane owns f and f+64), register accumulators,
    // 8 edges per batch: 16 independent row loads in flight per lane.
    // Lanes past the row end read its last channel and do not store.
    for (int64_t fb = 0; fb < feat; fb += 2 * kWave) {
      const int64_t f0 = fb + lane, f1 = fb + lane + kWave;
      const int64_t g0 = f0 < feat ? f0 : feat - 1;
      const int64_t g1 = f1 < feat ? f1 : feat - 1;
      const bool two = fb + kWave < feat;  // wave-uniform
      float a0 = 0.f, a1 = 0.f;
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        int64_t cc[8];
        float cw[8], cf[8], v0[8], v1[8];
        wsum_edge_batch(col, kW ? w : nullptr, kB ? b : nullptr, k0, nb,
                        feat, cc, cw, cf);
#pragma unroll
        for (int q = 0; q < 8; ++q) cf[q] *= cw[q];
#pragma unroll
        for (int q = 0; q < 8; ++q)
          v0[q] = static_cast<float>(x[cc[q] + g0]);
        if (two) {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            v1[q] = static_cast<float>(x[cc[q] + g1]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) a0 += q < nb ? cf[q] * v0[q] : 0.f;
        if (two) {
#pragma unroll
          for (int q = 0; q < 8; ++q) a1 += q < nb ? cf[q] * v1[q] : 0.f;
        }
      }
      if (f0 < feat) out[t * feat + f0] = static_cast<scalar_t>(a0 * at);
      if (f1 < feat) out[t * feat + f1] = static_cast<scalar_t>(a1 * at);
    }
  }
}

// bf16 fast path for even F: each lane owns two adjacent channels (one
// 4-byte load per row visit), 64 pairs per pass.
template <bool kW, bool kB>
__global__ void seg_wsum_fwd_bf162_kernel(
    const __hip_bfloat162* __restrict__ x, const int64_t* __restrict__ col,
    const int64_t* __restrict__ off, const float* __restrict__ w,
    const float* __restrict__ a, const float* __restrict__ b, int64_t n_tgt,
    int64_t feat2, __hip_bfloat162* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    const float at = a != nullptr ? a[t] : 1.0f;
    for (int64_t fb = 0; fb < feat2; fb += kWave) {
      const int64_t f = fb + lane;
      const int64_t g = f < feat2 ? f : feat2 - 1;
      float2 acc = {0.f, 0.f};
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        int64_t cc[8];
        float cw[8], cf[8];
        __hip_bfloat162 v[8];
        wsum_edge_batch(col, kW ? w : nullptr, kB ? b : nullptr, k0, nb,
                        feat2, cc, cw, cf);
#pragma unroll
        for (int q = 0; q < 8; ++q) cf[q] *= cw[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = x[cc[q] + g];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float2 u = __bfloat1622float2(v[q]);
          acc.x += q < nb ? cf[q] * u.x : 0.f;
          acc.y += q < nb ? cf[q] * u.y : 0.f;
        }
      }
      if (f < feat2)
        out[t * feat2 + f] =
            __float22bfloat162_rn({acc.x * at, acc.y * at});
    }
  }
}

// Backward of the weighted segment sum, for every edge e = (t, c):
//   kDx: dx[c, :] += a[t] * w[e] * b[c] * dy[t, :]   (fp32 atomics, arena)
//   kDw: dw[e]     = a[t] * b[c] * <dy[t, :], x[c, :]>
// dw is a per-edge wave dot product (xor-shuffle reduction) written with
// one plain store per edge: no atomics, so it is the same bits every run.
// Without kDw x is never read.  In order-independent mode the terms are
// bounded by max|dy| * coef_bound (coef_bound >= max|a| max|w| max|b|), so
// the grid exponent comes from that product.
template <typename scalar_t, bool kDx, bool kDw>
__global__ void seg_wsum_bwd_kernel(const scalar_t* __restrict__ dy,
                                    const scalar_t* __restrict__ x,
                                    const int64_t* __restrict__ col,
                                    const int64_t* __restrict__ off,
                                    const float* __restrict__ w,
                                    const float* __restrict__ a,
                                    const float* __restrict__ b,
                                    int64_t n_tgt, int64_t feat,
                                    const float* __restrict__ amax_parts,
                                    int n_parts,
                                    const float* __restrict__ coef_bound,
                                    float* __restrict__ dx,
                                    float* __restrict__ dw) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const float magic =
      kDx ? grid_magic(amax_parts, n_parts, coef_bound) : 0.f;
  const bool in_regs = feat <= 2 * kWave;
  const bool two = feat > kWave;
  const int64_t f0 = lane, f1 = lane + kWave;
  // clamped channels: x loads for dw are issued for all 64 lanes
  const int64_t c0 = f0 < feat ? f0 : feat - 1;
  const int64_t c1 = f1 < feat ? f1 : feat - 1;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    if (e <= s) continue;
    const float at = a != nullptr ? a[t] : 1.0f;
    // the dy row is shared by every edge of the segment
    float g0 = 0.f, g1 = 0.f;
    if (in_regs) {
      if (f0 < feat) g0 = static_cast<float>(dy[t * feat + f0]);
      if (f1 < feat) g1 = static_cast<float>(dy[t * feat + f1]);
    }
    for (int64_t k0 = s; k0 < e; k0 += 8) {
      const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
      int64_t cc[8];
      float cw[8], cb[8];
      wsum_edge_batch(col, w, b, k0, nb, feat, cc, cw, cb);
      float x0[8], x1[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) x0[q] = x1[q] = 0.f;
      if (kDw && in_regs) {  // 8 (16) independent row loads in flight
#pragma unroll
        for (int q = 0; q < 8; ++q)
          x0[q] = static_cast<float>(x[cc[q] + c0]);
        if (two) {
#pragma unroll
          for (int q = 0; q < 8; ++q)
            x1[q] = static_cast<float>(x[cc[q] + c1]);
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (q < nb) {  // wave-uniform
          const float ab = at * cb[q];
          const float coef = ab * cw[q];
          float dot = 0.f;
          if (in_regs) {
            if (f0 < feat) {
              if (kDx) atomicAdd(&dx[cc[q] + f0], snap(g0 * coef, magic));
              if (kDw) dot += g0 * x0[q];
            }
            if (f1 < feat) {
              if (kDx) atomicAdd(&dx[cc[q] + f1], snap(g1 * coef, magic));
              if (kDw) dot += g1 * x1[q];
            }
          } else {
            for (int64_t f = lane; f < feat; f += kWave) {
              const float g = static_cast<float>(dy[t * feat + f]);
              if (kDx) atomicAdd(&dx[cc[q] + f], snap(g * coef, magic));
              if (kDw) dot += g * static_cast<float>(x[cc[q] + f]);
            }
          }
          if (kDw) {
            for (int o = kWave / 2; o > 0; o >>= 1)
              dot += __shfl_xor(dot, o, kWave);
            if (lane == 0) dw[k0 + q] = ab * dot;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Segment max / min with the arg of the winner (torch_scatter rule):
//   out[t, f] = max (min) over e in [off[t], off[t+1]) of x[col[e], f]
//   arg[t, f] = col[e*], e* the FIRST edge of the segment, in edge order,
//               that attains it
// The running winner starts as the first edge of the segment (no +-inf or
// zero sentinel) and is replaced only on a strict compare, so ties keep
// the earlier edge; a NaN replaces any non-NaN winner and then stays (NaN
// compares false), so arg is the first NaN edge.  An empty segment gives
// out = 0, arg = -1.  The forward is a selection: compares run in fp32
// (exact for bf16 input) and the winner's own bits are stored.
// kCat: out is [n_tgt, 2F] with out[t, F:] = x[t, :], as in the mean family.
// kArg = false stores no arg (x needs no gradient).
// Backward: dx[arg[t, f], f] += dy[t, f], exactly one source row per
// output element (and dx[t, :] += dy[t, F:] with kCat).
// ---------------------------------------------------------------------------

template <bool kMax>
__device__ __forceinline__ bool ext_wins(float v, float best) {
  return (kMax ? v > best : v < best) || (v != v && best == best);
}

// Source rows of up to 8 edges starting at k0, in scalar registers.  Slots
// past the end of the segment repeat edge k0 (a valid row), so the row
// loads need no branch; the caller masks them by q < nb.
__device__ __forceinline__ void ext_edge_batch(const int64_t* __restrict__ col,
                                               int64_t k0, int nb,
                                               int64_t (&c)[8]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) c[q] = col[q < nb ? k0 + q : k0];
}

__device__ __forceinline__ float ext_value(float v) { return v; }
__device__ __forceinline__ float ext_value(c10::BFloat16 v) {
  return __uint_as_float((uint32_t)v.x << 16);
}

template <typename scalar_t, bool kMax, bool kCat, bool kArg>
__global__ void seg_ext_fwd_kernel(const scalar_t* __restrict__ x,
                                   const int64_t* __restrict__ col,
                                   const int64_t* __restrict__ off,
                                   int64_t n_tgt, int64_t feat,
                                   scalar_t* __restrict__ out,
                                   int32_t* __restrict__ arg) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * feat : feat;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    // 128 channels per pass (lane owns f and f+64), 8 edges per batch.
    // Lanes past the row end read its last channel and do not store.
    for (int64_t fb = 0; fb < feat; fb += 2 * kWave) {
      const int64_t f0 = fb + lane, f1 = fb + lane + kWave;
      const int64_t g0 = f0 < feat ? f0 : feat - 1;
      const int64_t g1 = f1 < feat ? f1 : feat - 1;
      const bool two = fb + kWave < feat;  // wave-uniform
      scalar_t w0 = static_cast<scalar_t>(0.f), w1 = w0;  // winner's bits
      float m0 = 0.f, m1 = 0.f;
      int32_t i0 = -1, i1 = -1;
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        const bool first = k0 == s;  // slot 0 of the first batch always wins
        int64_t c[8];
        scalar_t v0[8], v1[8];
        ext_edge_batch(col, k0, nb, c);
#pragma unroll
        for (int q = 0; q < 8; ++q) v0[q] = x[c[q] * feat + g0];
        if (two) {
#pragma unroll
          for (int q = 0; q < 8; ++q) v1[q] = x[c[q] * feat + g1];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float u = ext_value(v0[q]);
          if (q < nb && ((q == 0 && first) || ext_wins<kMax>(u, m0))) {
            m0 = u;
            w0 = v0[q];
            i0 = (int32_t)c[q];
          }
        }
        if (two) {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float u = ext_value(v1[q]);
            if (q < nb && ((q == 0 && first) || ext_wins<kMax>(u, m1))) {
              m1 = u;
              w1 = v1[q];
              i1 = (int32_t)c[q];
            }
          }
        }
      }
      if (f0 < feat) {
        out[t * ostride + f0] = w0;
        if constexpr (kArg) arg[t * feat + f0] = i0;
        if constexpr (kCat) out[t * ostride + feat + f0] = x[t * feat + f0];
      }
      if (f1 < feat) {
        out[t * ostride + f1] = w1;
        if constexpr (kArg) arg[t * feat + f1] = i1;
        if constexpr (kCat) out[t * ostride + feat + f1] = x[t * feat + f1];
      }
    }
  }
}

// bf16 fast path for even F: a lane owns one adjacent channel pair, so a
// row visit is one 4-byte load and the arg pair one 8-byte store (t * F +
// 2f is even).  The pair travels as its raw 32 bits: low half = channel
// 2f, high half = channel 2f + 1.
template <bool kMax, bool kCat, bool kArg>
__global__ void seg_ext_fwd_bf162_kernel(const uint32_t* __restrict__ x,
                                         const int64_t* __restrict__ col,
                                         const int64_t* __restrict__ off,
                                         int64_t n_tgt, int64_t feat2,
                                         uint32_t* __restrict__ out,
                                         int2* __restrict__ arg) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = wave_uniform(
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave);
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ostride = kCat ? 2 * feat2 : feat2;
  for (int64_t t = wave; t < n_tgt; t += n_waves) {
    const int64_t s = off[t], e = off[t + 1];
    for (int64_t fb = 0; fb < feat2; fb += kWave) {
      const int64_t f = fb + lane;
      const int64_t g = f < feat2 ? f : feat2 - 1;
      uint32_t wlo = 0, whi = 0;  // winner's bits, each in its own half
      float mlo = 0.f, mhi = 0.f;
      int2 idx = {-1, -1};
      for (int64_t k0 = s; k0 < e; k0 += 8) {
        const int nb = (int)((e - k0) < 8 ? (e - k0) : 8);
        const bool first = k0 == s;
        int64_t c[8];
        uint32_t v[8];
        ext_edge_batch(col, k0, nb, c);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = x[c[q] * feat2 + g];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float ulo = __uint_as_float(v[q] << 16);
          const float uhi = __uint_as_float(v[q] & 0xffff0000u);
          const bool take = q == 0 && first;
          if (q < nb && (take || ext_wins<kMax>(ulo, mlo))) {
            mlo = ulo;
            wlo = v[q] & 0xffffu;
            idx.x = (int32_t)c[q];
          }
          if (q < nb && (take || ext_wins<kMax>(uhi, mhi))) {
            mhi = uhi;
            whi = v[q] & 0xffff0000u;
            idx.y = (int32_t)c[q];
          }
        }
      }
      if (f < feat2) {
        out[t * ostride + f] = wlo | whi;
        if constexpr (kArg) arg[t * feat2 + f] = idx;
        if constexpr (kCat) out[t * ostride + feat2 + f] = x[t * feat2 + f];
      }
    }
  }
}

// One lane per (t, f): dx[arg[t, f], f] += dy[t, f] where arg >= 0, plus
// the root term with kCat.  Several targets may pick the same source row,
// hence the atomics; the terms are the dy values themselves, so the
// order-independent grid needs no scale.  Reads neither col nor offsets.
template <typename scalar_t, bool kCat>
__global__ void seg_ext_bwd_kernel(const scalar_t* __restrict__ dy,
                                   const int32_t* __restrict__ arg,
                                   int64_t n_tgt, int64_t feat,
                                   const float* __restrict__ amax_parts,
                                   int n_parts, float* __restrict__ dx) {
  const float magic = grid_magic(amax_parts, n_parts);
  const int64_t total = n_tgt * feat;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t ostride = kCat ? 2 * feat : feat;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t t = i / feat, f = i - t * feat;
    const int32_t a = arg[i];
    if (a >= 0)
      atomicAdd(&dx[(int64_t)a * feat + f],
                snap(static_cast<float>(dy[t * ostride + f]), magic));
    if constexpr (kCat)
      atomicAdd(&dx[i],
                snap(static_cast<float>(dy[t * ostride + feat + f]), magic));
  }
}

int wave_grid(int64_t rows) {
  const int64_t waves = std::min<int64_t>(rows, (int64_t)kMaxBlocks * 4);
  return (int)std::min<int64_t>((waves * kWave + kBlock - 1) / kBlock,
                                kMaxBlocks);
}

#define GLT_DISPATCH_SEG(TYPE, NAME, ...)                          \
  [&] {                                                            \
    switch (TYPE) {                                                \
      case torch::kFloat32: {                                      \
        using scalar_t = float;                                    \
        return __VA_ARGS__();                                      \
      }                                                            \
      case torch::kBFloat16: {                                     \
        using scalar_t = c10::BFloat16;                            \
        return __VA_ARGS__();                                      \
      }                                                            \
      default:                                                     \
        TORCH_CHECK(false, NAME ": unsupported dtype (fp32/bf16)");\
    }                                                              \
  }()

// x or dy of an entry point: [rows, F], fp32 or bf16, on the device
void check_values(const torch::Tensor& v, const char* what,
                  bool contiguous) {
  TORCH_CHECK(v.is_cuda() && v.dim() == 2 &&
                  (v.scalar_type() == torch::kFloat32 ||
                   v.scalar_type() == torch::kBFloat16),
              "segment: ", what, " must be a 2-D fp32/bf16 tensor on device");
  TORCH_CHECK(!contiguous || v.is_contiguous(),
              "segment: ", what, " must be contiguous");
}

// col / offsets of an entry point: the kernels read offsets[0 .. n_tgt]
// and col[offsets[0] .. offsets[n_tgt])
void check_index(const torch::Tensor& col, const torch::Tensor& offsets,
                 int64_t n_tgt) {
  TORCH_CHECK(col.is_cuda() && col.is_contiguous() &&
                  col.scalar_type() == torch::kInt64 && offsets.is_cuda() &&
                  offsets.is_contiguous() &&
                  offsets.scalar_type() == torch::kInt64,
              "segment: col/offsets must be contiguous int64 on device");
  TORCH_CHECK(n_tgt >= 0 && offsets.numel() == n_tgt + 1,
              "segment: offsets must have n_tgt + 1 entries");
}

template <bool kCat>
torch::Tensor segment_mean_fwd(const torch::Tensor& x,
                               const torch::Tensor& col,
                               const torch::Tensor& offsets, int64_t n_tgt) {
  check_values(x, "x", true);
  check_index(col, offsets, n_tgt);
  TORCH_CHECK(!kCat || x.size(0) >= n_tgt,
              "segment_mean_cat: targets must be a row prefix of x");
  const int64_t feat = x.size(1);
  auto out = torch::empty({n_tgt, kCat ? 2 * feat : feat}, x.options());
  if (n_tgt == 0 || feat == 0) return out;
  if (x.scalar_type() == torch::kBFloat16 && feat % 2 == 0) {
    hipLaunchKernelGGL(seg_mean_fwd_bf162_kernel<kCat>,
                       dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                       current_stream(),
                       reinterpret_cast<const __hip_bfloat162*>(x.data_ptr()),
                       col.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       n_tgt, feat / 2,
                       reinterpret_cast<__hip_bfloat162*>(out.data_ptr()));
    return out;
  }
  GLT_DISPATCH_SEG(x.scalar_type(), "segment_mean_fwd", [&] {
    hipLaunchKernelGGL((seg_mean_fwd_kernel<scalar_t, kCat>),
                       dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                       current_stream(), x.data_ptr<scalar_t>(),
                       col.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       n_tgt, feat, out.data_ptr<scalar_t>());
  });
  return out;
}

// fp32 accumulation arena [n_src, feat]; in order-independent mode it is
// followed by the block maxima of |dy|, and zero_absmax_kernel zeroes
// the first and fills the second.
struct BwdArena {
  torch::Tensor dx;
  float* parts;
  int n_parts;
};

template <typename scalar_t>
BwdArena make_bwd_arena(const torch::Tensor& dyc, int64_t n_src,
                        int64_t feat, bool order_independent) {
  if (!order_independent)  // plain mode: zero fill, no grid (n_parts == 0)
    return {torch::zeros({n_src, feat},
                         dyc.options().dtype(torch::kFloat32)),
            nullptr, 0};
  const int64_t n_arena = n_src * feat, n = dyc.numel();
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(
      (std::max(n_arena / 4, n) + kZeroBlock - 1) / kZeroBlock,
      kMaxAmaxParts));
  auto flat = torch::empty({n_arena + blocks},
                           dyc.options().dtype(torch::kFloat32));
  float* base = flat.data_ptr<float>();
  hipLaunchKernelGGL(zero_absmax_kernel<scalar_t>, dim3(blocks),
                     dim3(kZeroBlock), 0, current_stream(), base, n_arena,
                     dyc.data_ptr<scalar_t>(), n, base + n_arena);
  return {flat.narrow(0, 0, n_arena).view({n_src, feat}), base + n_arena,
          blocks};
}

// Returns fp32 regardless of dy dtype (fp32 atomic accumulation arena);
// the python wrapper casts to dy.dtype once.
template <bool kCat>
torch::Tensor segment_mean_bwd(const torch::Tensor& dy,
                               const torch::Tensor& col,
                               const torch::Tensor& offsets, int64_t n_src,
                               bool order_independent) {
  check_values(dy, "dy", false);
  const int64_t n_tgt = dy.size(0);
  check_index(col, offsets, n_tgt);
  if (kCat) {
    TORCH_CHECK(dy.size(1) % 2 == 0,
                "segment_mean_cat: dy must have an even number of columns");
    TORCH_CHECK(n_src >= n_tgt,
                "segment_mean_cat: targets must be a row prefix of x");
  }
  const int64_t feat = kCat ? dy.size(1) / 2 : dy.size(1);
  if (n_tgt == 0 || feat == 0)
    return torch::zeros({n_src, feat}, dy.options().dtype(torch::kFloat32));
  auto dyc = dy.contiguous();
  torch::Tensor dx;
  GLT_DISPATCH_SEG(dy.scalar_type(), "segment_mean_bwd", [&] {
    auto arena = make_bwd_arena<scalar_t>(dyc, n_src, feat,
                                          order_independent);
    dx = arena.dx;
    hipLaunchKernelGGL((seg_mean_bwd_kernel<scalar_t, kCat>),
                       dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                       current_stream(), dyc.data_ptr<scalar_t>(),
                       col.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       n_tgt, feat, arena.parts, arena.n_parts,
                       dx.data_ptr<float>());
  });
  return dx;
}

// runtime bool -> compile-time flag: fn(std::true_type{} / std::false_type{})
template <typename Fn>
void with_flag(bool v, Fn&& fn) {
  if (v)
    fn(std::true_type{});
  else
    fn(std::false_type{});
}

// 1-D contiguous int64 index tensor on the device
void check_index_1d(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.is_contiguous() &&
                  t.scalar_type() == torch::kInt64,
              "segment: ", what, " must be a contiguous 1-D int64 tensor on "
              "device");
}

// consecutive sources per wave of the gather backward: 1, 2, 4 and 8 were
// measured at the flagship shapes and 1 was fastest (docs/kernels.md)
constexpr int kGatherRows = 1;

template <typename P, bool kCat, int kRows>
void segment_mean_bwd_gather_launch(const torch::Tensor& dyc,
                                    const torch::Tensor& offsets,
                                    const torch::Tensor& src_off,
                                    const torch::Tensor& in_tgt,
                                    const torch::Tensor* mask, int64_t n_src,
                                    int64_t units, const float* parts,
                                    int n_parts, torch::Tensor& out) {
  using unit_t = typename P::unit_t;
  const int64_t n_blk = (n_src + kRows - 1) / kRows;
  with_flag(mask != nullptr, [&](auto kMask) {
    hipLaunchKernelGGL(
        (seg_mean_bwd_gather_kernel<P, kCat, decltype(kMask)::value, kRows>),
        dim3(wave_grid(n_blk)), dim3(kBlock), 0, current_stream(),
        reinterpret_cast<const unit_t*>(dyc.data_ptr()),
        offsets.data_ptr<int64_t>(), src_off.data_ptr<int64_t>(),
        in_tgt.data_ptr<int64_t>(),
        mask ? reinterpret_cast<const unit_t*>(mask->data_ptr()) : nullptr,
        dyc.size(0), n_src, units, parts, n_parts,
        reinterpret_cast<unit_t*>(out.data_ptr()));
  });
}

// dx [n_src, F] in dy's dtype, every row written by the kernel
template <bool kCat>
torch::Tensor segment_mean_bwd_gather(
    const torch::Tensor& dy, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_src, bool order_independent,
    const torch::Tensor& src_off, const torch::Tensor& in_tgt,
    const c10::optional<torch::Tensor>& mask) {
  check_values(dy, "dy", false);
  const int64_t n_tgt = dy.size(0);
  check_index(col, offsets, n_tgt);
  if (kCat) {
    TORCH_CHECK(dy.size(1) % 2 == 0,
                "segment_mean_cat: dy must have an even number of columns");
    TORCH_CHECK(n_src >= n_tgt,
                "segment_mean_cat: targets must be a row prefix of x");
  }
  const int64_t feat = kCat ? dy.size(1) / 2 : dy.size(1);
  check_index_1d(src_off, "src_off");
  check_index_1d(in_tgt, "in_edge");
  TORCH_CHECK(n_src >= 0 && src_off.numel() == n_src + 1 &&
                  in_tgt.numel() == col.numel(),
              "segment: src_off must have n_src + 1 entries and in_edge one "
              "per edge (segment_transpose(col, n_src, tgt))");
  if (mask.has_value())
    TORCH_CHECK(mask->is_cuda() && mask->dim() == 2 &&
                    mask->is_contiguous() && mask->size(0) >= n_src &&
                    mask->size(1) == feat &&
                    mask->scalar_type() == dy.scalar_type(),
                "segment: mask must be a contiguous [>= n_src, F] tensor of "
                "dy's dtype on device");
  if (n_tgt == 0 || feat == 0 || n_src == 0)
    return torch::zeros({n_src, feat}, dy.options());
  auto dyc = dy.contiguous();
  auto out = torch::empty({n_src, feat}, dy.options());
  const torch::Tensor* mp = mask.has_value() ? &*mask : nullptr;
  torch::Tensor parts_t;  // block maxima of |dy|: the order-independent grid
  float* parts = nullptr;
  int n_parts = 0;
  if (order_independent) {
    const int64_t n = dyc.numel();
    n_parts = (int)std::min<int64_t>((n + kZeroBlock - 1) / kZeroBlock,
                                     kMaxAmaxParts);
    parts_t = torch::empty({n_parts}, dy.options().dtype(torch::kFloat32));
    parts = parts_t.data_ptr<float>();
    GLT_DISPATCH_SEG(dy.scalar_type(), "segment_mean_bwd_gather", [&] {
      hipLaunchKernelGGL(zero_absmax_kernel<scalar_t>, dim3(n_parts),
                         dim3(kZeroBlock), 0, current_stream(),
                         (float*)nullptr, (int64_t)0,
                         dyc.data_ptr<scalar_t>(), n, parts);
    });
  }
#define GLT_GATHER(P, UNITS)                                          \
  segment_mean_bwd_gather_launch<P, kCat, kGatherRows>(               \
      dyc, offsets, src_off, in_tgt, mp, n_src, UNITS, parts, n_parts, out)
  const bool bf16 = dy.scalar_type() == torch::kBFloat16;
  // the wide units need their alignment (a view may start anywhere)
  const uintptr_t addr = (uintptr_t)dyc.data_ptr() | (uintptr_t)out.data_ptr() |
                         (mp ? (uintptr_t)mp->data_ptr() : 0);
  if (bf16 && feat % 4 == 0 && addr % 8 == 0)
    GLT_GATHER(GatherBf164, feat / 4);
  else if (bf16 && feat % 2 == 0 && addr % 4 == 0)
    GLT_GATHER(GatherBf162, feat / 2);
  else if (!bf16 && feat % 4 == 0 && addr % 16 == 0)
    GLT_GATHER(GatherF324, feat / 4);
  else if (bf16)
    GLT_GATHER(GatherScalar<c10::BFloat16>, feat);
  else
    GLT_GATHER(GatherScalar<float>, feat);
#undef GLT_GATHER
  return out;
}

template <bool kMax, bool kCat, bool kArg>
void segment_ext_fwd_launch(const torch::Tensor& x, const torch::Tensor& col,
                            const torch::Tensor& offsets, int64_t n_tgt,
                            torch::Tensor& out, int32_t* argp) {
  const int64_t feat = x.size(1);
  if (x.scalar_type() == torch::kBFloat16 && feat % 2 == 0) {
    hipLaunchKernelGGL((seg_ext_fwd_bf162_kernel<kMax, kCat, kArg>),
                       dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                       current_stream(),
                       reinterpret_cast<const uint32_t*>(x.data_ptr()),
                       col.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       n_tgt, feat / 2,
                       reinterpret_cast<uint32_t*>(out.data_ptr()),
                       reinterpret_cast<int2*>(argp));
    return;
  }
  GLT_DISPATCH_SEG(x.scalar_type(), "segment_ext_fwd", [&] {
    hipLaunchKernelGGL((seg_ext_fwd_kernel<scalar_t, kMax, kCat, kArg>),
                       dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                       current_stream(), x.data_ptr<scalar_t>(),
                       col.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       n_tgt, feat, out.data_ptr<scalar_t>(), argp);
  });
}

// optional fp32 factor of the weighted segment sum -> device pointer
const float* wsum_factor(const c10::optional<torch::Tensor>& t, int64_t n,
                         const char* what) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                  t->scalar_type() == torch::kFloat32 && t->numel() == n,
              "segment_wsum: ", what, " must be contiguous fp32 on device "
              "with ", n, " elements");
  return t->data_ptr<float>();
}

}  // namespace

torch::Tensor hip_segment_mean_fwd(const torch::Tensor& x,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   int64_t n_tgt) {
  return segment_mean_fwd<false>(x, col, offsets, n_tgt);
}

torch::Tensor hip_segment_mean_cat_fwd(const torch::Tensor& x,
                                       const torch::Tensor& col,
                                       const torch::Tensor& offsets,
                                       int64_t n_tgt) {
  return segment_mean_fwd<true>(x, col, offsets, n_tgt);
}

torch::Tensor hip_segment_mean_bwd(const torch::Tensor& dy,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   int64_t n_src, bool order_independent) {
  return segment_mean_bwd<false>(dy, col, offsets, n_src, order_independent);
}

torch::Tensor hip_segment_mean_cat_bwd(const torch::Tensor& dy,
                                       const torch::Tensor& col,
                                       const torch::Tensor& offsets,
                                       int64_t n_src,
                                       bool order_independent) {
  return segment_mean_bwd<true>(dy, col, offsets, n_src, order_independent);
}

// Inverted index of col: (src_off int64 [n_src + 1], in_edge int64 [E]).
// in_edge[src_off[s] : src_off[s + 1]] lists the edges e with col[e] == s
// in ascending e (stable sort): as tgt[e] when tgt is given (what the
// gather backward reads), as the position e otherwise.  A stable rocprim
// radix_sort_pairs over the low ceil(log2(n_src)) key bits and one
// boundary kernel; scratch from the caching allocator, no host sync.
std::tuple<torch::Tensor, torch::Tensor> hip_segment_transpose(
    const torch::Tensor& col, int64_t n_src,
    const c10::optional<torch::Tensor>& tgt) {
  check_index_1d(col, "col");
  const int64_t n_edge = col.numel();
  TORCH_CHECK(n_src >= 0, "segment_transpose: n_src must be >= 0");
  if (tgt.has_value()) {
    check_index_1d(*tgt, "tgt");
    TORCH_CHECK(tgt->numel() == n_edge,
                "segment_transpose: tgt must have one entry per edge");
  }
  if (n_edge == 0)
    return {torch::zeros({n_src + 1}, col.options()),
            torch::empty({0}, col.options())};
  TORCH_CHECK(n_src > 0, "segment_transpose: edges but no source rows");
  auto src_off = torch::empty({n_src + 1}, col.options());
  auto in_edge = torch::empty({n_edge}, col.options());
  auto keys = torch::empty({n_edge}, col.options());
  const torch::Tensor values =
      tgt.has_value() ? *tgt : torch::arange(n_edge, col.options());
  unsigned bits = 1;  // 0 <= col < n_src: only these key bits differ
  while (bits < 63 && ((int64_t)1 << bits) < n_src) ++bits;
  hipStream_t stream = current_stream();
  // below 2^20 items rocprim takes its merge sort; forcing Onesweep was
  // measured slower at the flagship sizes (docs/kernels.md)
  size_t bytes = 0;
  GLT_HIP_CHECK(rocprim::radix_sort_pairs(
      nullptr, bytes, col.data_ptr<int64_t>(), keys.data_ptr<int64_t>(),
      values.data_ptr<int64_t>(), in_edge.data_ptr<int64_t>(),
      (size_t)n_edge, 0u, bits, stream));
  auto tmp = scratch_bytes((int64_t)std::max<size_t>(bytes, 1), col.device());
  GLT_HIP_CHECK(rocprim::radix_sort_pairs(
      tmp.data_ptr(), bytes, col.data_ptr<int64_t>(),
      keys.data_ptr<int64_t>(), values.data_ptr<int64_t>(),
      in_edge.data_ptr<int64_t>(), (size_t)n_edge, 0u, bits, stream));
  hipLaunchKernelGGL(seg_boundary_kernel,
                     dim3(grid_for(std::max(n_edge, n_src + 1))),
                     dim3(kBlock), 0, stream, keys.data_ptr<int64_t>(),
                     n_edge, n_src, src_off.data_ptr<int64_t>());
  return {src_off, in_edge};
}

torch::Tensor hip_segment_mean_bwd_gather(
    const torch::Tensor& dy, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_src, bool order_independent,
    const torch::Tensor& src_off, const torch::Tensor& in_edge,
    const c10::optional<torch::Tensor>& mask) {
  return segment_mean_bwd_gather<false>(dy, col, offsets, n_src,
                                        order_independent, src_off, in_edge,
                                        mask);
}

torch::Tensor hip_segment_mean_cat_bwd_gather(
    const torch::Tensor& dy, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_src, bool order_independent,
    const torch::Tensor& src_off, const torch::Tensor& in_edge,
    const c10::optional<torch::Tensor>& mask) {
  return segment_mean_bwd_gather<true>(dy, col, offsets, n_src,
                                       order_independent, src_off, in_edge,
                                       mask);
}

// (out, arg): out is [n_tgt, F] ([n_tgt, 2F] with cat) in x's dtype, arg is
// int32 [n_tgt, F] or None without need_arg.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> hip_segment_ext_fwd(
    const torch::Tensor& x, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_tgt, bool is_max, bool cat,
    bool need_arg) {
  check_values(x, "x", true);
  check_index(col, offsets, n_tgt);
  TORCH_CHECK(x.size(0) <= (int64_t)INT32_MAX,
              "segment_ext: arg is int32, x must have fewer than 2^31 rows");
  TORCH_CHECK(!cat || x.size(0) >= n_tgt,
              "segment_ext: cat needs the targets as a row prefix of x");
  const int64_t feat = x.size(1);
  auto out = torch::empty({n_tgt, cat ? 2 * feat : feat}, x.options());
  c10::optional<torch::Tensor> arg;
  if (need_arg)
    arg = torch::empty({n_tgt, feat}, x.options().dtype(torch::kInt32));
  if (n_tgt == 0 || feat == 0) return {out, arg};
  int32_t* argp = need_arg ? arg->data_ptr<int32_t>() : nullptr;
  with_flag(is_max, [&](auto kMax) {
    with_flag(cat, [&](auto kCat) {
      with_flag(need_arg, [&](auto kArg) {
        segment_ext_fwd_launch<decltype(kMax)::value, decltype(kCat)::value,
                               decltype(kArg)::value>(x, col, offsets, n_tgt,
                                                      out, argp);
      });
    });
  });
  return {out, arg};
}

// fp32 dx [n_src, F] (accumulation arena; the python wrapper casts once)
torch::Tensor hip_segment_ext_bwd(const torch::Tensor& dy,
                                  const torch::Tensor& arg, int64_t n_src,
                                  bool cat, bool order_independent) {
  check_values(dy, "dy", false);
  const int64_t n_tgt = dy.size(0);
  TORCH_CHECK(!cat || dy.size(1) % 2 == 0,
              "segment_ext: cat needs a dy with an even number of columns");
  const int64_t feat = cat ? dy.size(1) / 2 : dy.size(1);
  TORCH_CHECK(n_src >= 0 && n_src <= (int64_t)INT32_MAX &&
                  (!cat || n_src >= n_tgt),
              "segment_ext: n_src must be below 2^31 and, with cat, at "
              "least n_tgt");
  TORCH_CHECK(arg.is_cuda() && arg.is_contiguous() &&
                  arg.scalar_type() == torch::kInt32 && arg.dim() == 2 &&
                  arg.size(0) == n_tgt && arg.size(1) == feat,
              "segment_ext: arg must be a contiguous int32 [n_tgt, F] "
              "tensor on device");
  if (n_tgt == 0 || feat == 0)
    return torch::zeros({n_src, feat}, dy.options().dtype(torch::kFloat32));
  auto dyc = dy.contiguous();
  torch::Tensor dx;
  GLT_DISPATCH_SEG(dy.scalar_type(), "segment_ext_bwd", [&] {
    auto arena = make_bwd_arena<scalar_t>(dyc, n_src, feat,
                                          order_independent);
    dx = arena.dx;
    with_flag(cat, [&](auto kCat) {
      hipLaunchKernelGGL(
          (seg_ext_bwd_kernel<scalar_t, decltype(kCat)::value>),
          dim3(grid_for(n_tgt * feat)), dim3(kBlock), 0, current_stream(),
          dyc.data_ptr<scalar_t>(), arg.data_ptr<int32_t>(), n_tgt, feat,
          arena.parts, arena.n_parts, dx.data_ptr<float>());
    });
  });
  return dx;
}

// absent edge weight / source scale -> compile-time flags (no ones tensor,
// no per-edge branch)
#define GLT_WSUM_FLAGS(HAS_W, HAS_B, ...)                 \
  [&] {                                                   \
    if (HAS_W) {                                          \
      constexpr bool kW = true;                           \
      if (HAS_B) {                                        \
        constexpr bool kB = true;                         \
        return __VA_ARGS__();                             \
      }                                                   \
      constexpr bool kB = false;                          \
      return __VA_ARGS__();                               \
    }                                                     \
    constexpr bool kW = false;                            \
    if (HAS_B) {                                          \
      constexpr bool kB = true;                           \
      return __VA_ARGS__();                               \
    }                                                     \
    constexpr bool kB = false;                            \
    return __VA_ARGS__();                                 \
  }()

torch::Tensor hip_segment_wsum_fwd(const torch::Tensor& x,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   const c10::optional<torch::Tensor>& w,
                                   const c10::optional<torch::Tensor>& a,
                                   const c10::optional<torch::Tensor>& b) {
  check_values(x, "x", true);
  const int64_t n_tgt = offsets.numel() - 1;
  const int64_t feat = x.size(1);
  check_index(col, offsets, n_tgt);
  const float* wp = wsum_factor(w, col.numel(), "edge weight");
  const float* ap = wsum_factor(a, n_tgt, "target scale");
  const float* bp = wsum_factor(b, x.size(0), "source scale");
  auto out = torch::empty({n_tgt, feat}, x.options());
  if (n_tgt > 0 && feat > 0) {
    const bool hw = wp != nullptr, hb = bp != nullptr;
    if (x.scalar_type() == torch::kBFloat16 && feat % 2 == 0) {
      auto x2 = reinterpret_cast<const __hip_bfloat162*>(x.data_ptr());
      auto o2 = reinterpret_cast<__hip_bfloat162*>(out.data_ptr());
      GLT_WSUM_FLAGS(hw, hb, [&] {
        hipLaunchKernelGGL((seg_wsum_fwd_bf162_kernel<kW, kB>),
                           dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                           current_stream(), x2, col.data_ptr<int64_t>(),
                           offsets.data_ptr<int64_t>(), wp, ap, bp, n_tgt,
                           feat / 2, o2);
      });
      return out;
    }
    GLT_DISPATCH_SEG(x.scalar_type(), "segment_wsum_fwd", [&] {
      GLT_WSUM_FLAGS(hw, hb, [&] {
        hipLaunchKernelGGL((seg_wsum_fwd_kernel<scalar_t, kW, kB>),
                           dim3(wave_grid(n_tgt)), dim3(kBlock), 0,
                           current_stream(), x.data_ptr<scalar_t>(),
                           col.data_ptr<int64_t>(),
                           offsets.data_ptr<int64_t>(), wp, ap, bp, n_tgt,
                           feat, out.data_ptr<scalar_t>());
      });
    });
  }
  return out;
}

#define GLT_WSUM_BWD(DX, DW)                                              \
  hipLaunchKernelGGL((seg_wsum_bwd_kernel<scalar_t, DX, DW>),             \
                     dim3(wave_grid(n_tgt)), dim3(kBlock), 0,             \
                     current_stream(), dyc.data_ptr<scalar_t>(), xp,      \
                     col.data_ptr<int64_t>(),                             \
                     offsets.data_ptr<int64_t>(), wp, ap, bp, n_tgt,      \
                     feat, arena.parts, arena.n_parts, cbp, dxp, dwp)

// (dx, dw): dx is fp32 [n_src, F] (accumulation arena; the python wrapper
// casts once), dw is fp32 [E]; each is None unless asked for.  x is only
// needed (and only read) for dw.
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
hip_segment_wsum_bwd(const torch::Tensor& dy,
                     const c10::optional<torch::Tensor>& x,
                     const torch::Tensor& col, const torch::Tensor& offsets,
                     const c10::optional<torch::Tensor>& w,
                     const c10::optional<torch::Tensor>& a,
                     const c10::optional<torch::Tensor>& b, int64_t n_src,
                     bool need_dx, bool need_dw, bool order_independent,
                     const c10::optional<torch::Tensor>& coef_bound) {
  check_values(dy, "dy", false);
  const int64_t n_tgt = dy.size(0);
  const int64_t feat = dy.size(1);
  const int64_t n_edge = col.numel();
  check_index(col, offsets, n_tgt);
  const float* wp = wsum_factor(w, n_edge, "edge weight");
  const float* ap = wsum_factor(a, n_tgt, "target scale");
  const float* bp = wsum_factor(b, n_src, "source scale");
  const float* cbp = order_independent && need_dx
                         ? wsum_factor(coef_bound, 1, "coefficient bound")
                         : nullptr;
  if (need_dw)
    TORCH_CHECK(x.has_value() && x->is_cuda() && x->is_contiguous() &&
                    x->dim() == 2 && x->size(0) == n_src &&
                    x->size(1) == feat &&
                    x->scalar_type() == dy.scalar_type(),
                "segment_wsum_bwd: dw needs x as a contiguous [n_src, F] "
                "tensor of dy's dtype");
  const auto f32 = dy.options().dtype(torch::kFloat32);
  c10::optional<torch::Tensor> dx, dw;
  // zeros: edges past off[n_tgt] (targets >= n_tgt) get no gradient
  if (need_dw) dw = torch::zeros({n_edge}, f32);
  if (n_tgt == 0 || feat == 0 || n_edge == 0 || !(need_dx || need_dw)) {
    if (need_dx) dx = torch::zeros({n_src, feat}, f32);
    return {dx, dw};
  }
  auto dyc = dy.contiguous();
  GLT_DISPATCH_SEG(dy.scalar_type(), "segment_wsum_bwd", [&] {
    BwdArena arena{torch::Tensor(), nullptr, 0};
    if (need_dx) {
      arena = make_bwd_arena<scalar_t>(dyc, n_src, feat, order_independent);
      dx = arena.dx;
    }
    const scalar_t* xp = need_dw ? x->data_ptr<scalar_t>() : nullptr;
    float* dxp = need_dx ? arena.dx.data_ptr<float>() : nullptr;
    float* dwp = need_dw ? dw->data_ptr<float>() : nullptr;
    if (need_dx && need_dw)
      GLT_WSUM_BWD(true, true);
    else if (need_dx)
      GLT_WSUM_BWD(true, false);
    else
      GLT_WSUM_BWD(false, true);
  });
  return {dx, dw};
}
#undef GLT_WSUM_BWD

}  // namespace glt

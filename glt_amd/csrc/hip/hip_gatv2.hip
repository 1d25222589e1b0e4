/* Fused GATv2 ("dynamic" attention, Brody et al.) edge softmax + weighted
 * aggregation for gfx950, forward and an atomic-free backward.
 *
 * Edges sorted by target, t = tgt[e], s = src[e]; hl [Ns, H, C] is the
 * source projection, hr [Nt.., H, C] the target projection, att [H, C]:
 *
 *   u_e[h,c]   = hl[s,h,c] + hr[t,h,c]
 *   score_e[h] = sum_c att[h,c] * leaky_relu(u_e[h,c])
 *   p_e[h]     = softmax over seg(t) of score_e[h]
 *   out[t,h,:] = sum_{e in seg(t)} p_e[h] * hl[s,h,:]     (empty segment: 0)
 *
 *   ds_e    = p_e * (<dout_t, hl_s> - <dout_t, out_t>)
 *   g_e[c]  = ds_e * att[c] * (u_e[c] > 0 ? 1 : slope)
 *   dhl[s]  = sum_{e: src[e] = s} (p_e * dout_t + g_e)
 *   dhr[t]  = sum_{e in seg(t)} g_e
 *   datt[c] = sum_e ds_e * leaky_relu(u_e[c])
 *
 * Unlike v1 the score is not a sum of two per-node logits, so it is
 * computed per edge from the rows the aggregation loads anyway; the
 * [E, H, C] pre-activation never exists in memory.
 *
 * Forward: one wave per (target, head), each lane owns two channels, hr[t]
 * and att[h] stay in registers, row loads are batched 4 edges at a time,
 * the softmax runs online on scores held as float pairs (see struct ff).
 * It saves (out, m, Z) only; for a bf16 h that
 * will be differentiated it also keeps the unrounded fp32 out, because the
 * backward's <dout_t, out_t> taken from the rounded out would put a bf16
 * rounding error into every gradient.
 *
 * Backward, no float atomics, two passes:
 *   by target: one wave per (t, h) recomputes score_e (same code as the
 *     forward) and <dout_t, hl_s>, two interleaved wave
 *     reductions per edge; stores p_e and ds_e to [E, H] fp32 scratch with
 *     plain stores (and one shift per (t, h), see the kernel); sums
 *     dhr[t,h,:] in registers and stores it once in h's
 *     dtype; keeps datt partials per lane.  A wave keeps one head for its
 *     whole life, so its datt partial is one [C] row of a slab, which a
 *     small kernel sums per head in a fixed order.
 *   by source: one wave per (s, h) walks the in-edge list of s (edge ids
 *     in ascending e, from hip_segment_transpose), sums
 *     p_e * dout[t_e] + ds_e * att * leaky'(hl[s] + hr[t_e]) in fp32 and
 *     stores dhl[s,h,:] once in h's dtype; every row is written.
 * Every sum has a fixed order, so all gradients are run-to-run identical.
 *
 * Known limits: a (t, h) segment and a source's in-list are each summed by
 * one wave (no segment split for layers with few targets, no list split
 * for hub sources); the by-source pass runs as long as its most loaded
 * source.
 */
#include <hip/hip_bf16.h>

#include <type_traits>

#include "hip_wave.h"
#include "../include/common.h"

// The float-pair arithmetic below (two_sum, two_prod) is only error-free if
// a product is rounded where it is written: after inlining, contraction
// would fold a rounded product into the next add as an fma and break the
// pair.  The fmas that are wanted are written out (__fmaf_rn).
#pragma clang fp contract(off)

namespace glt {

namespace {

constexpr int kEb = 4;  // edges per load batch

__device__ __forceinline__ float leaky(float u, float slope) {
  return u > 0.f ? u : u * slope;
}

// The score is kept as an unevaluated sum of two floats, h + l with
// |l| << |h| (all fp32 operations; Dekker / Knuth error-free sums and
// fma-based products).  A plain fp32 score near 100 carries an error of
// several 1e-6, the ulp there is 7.6e-6, and where two scores of a segment
// nearly tie that error goes into p unreduced and from there, times att,
// into every gradient.  The pair is good to ~1e-12 of the score; only the
// difference to the segment maximum is rounded to one float, where it is
// small whenever p matters.
struct ff {
  float h, l;
};

__device__ __forceinline__ ff two_sum(float a, float b) {
  const float s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}

__device__ __forceinline__ ff two_prod(float a, float b) {
  const float p = a * b;
  return {p, __fmaf_rn(a, b, -p)};
}

// att * leaky_relu(x + r); the slope comes as the pair (sh, sl), so that a
// slope such as 0.2 is the caller's double and not its nearest float
__device__ __forceinline__ ff score_term(float x, float r, float a, float sh,
                                         float sl) {
  ff u = two_sum(x, r);
  if (!(u.h > 0.f)) {  // u.h = fl(x + r) has the sign of x + r
    const ff v = two_prod(sh, u.h);
    u = {v.h, v.l + (sh * u.l + sl * u.h)};
  }
  const ff t = two_prod(a, u.h);
  return {t.h, t.l + a * u.l};
}

// A lane's share of score_e; forward and backward both take it from here.
__device__ __forceinline__ ff score_part(float h0, float h1, float r0,
                                         float r1, float a0, float a1,
                                         float sh, float sl) {
  const ff t0 = score_term(h0, r0, a0, sh, sl);
  const ff t1 = score_term(h1, r1, a1, sh, sl);
  const ff s = two_sum(t0.h, t1.h);
  return {s.h, s.l + (t0.l + t1.l)};
}

// one level of the wave tree on a pair
__device__ __forceinline__ void ff_shfl_add(ff& v, int sft) {
  const float oh = __shfl_down(v.h, sft), ol = __shfl_down(v.l, sft);
  const ff s = two_sum(v.h, oh);
  v = {s.h, s.l + (v.l + ol)};
}

// lane 0's pair to every lane, normalised (h = fl(h + l))
__device__ __forceinline__ ff ff_bcast(const ff& v) {
  return two_sum(__shfl(v.h, 0), __shfl(v.l, 0));
}

// s += x with the rounding error carried in c: a hub segment's Z and out
// come out at an ulp or two however long it is.
__device__ __forceinline__ void kahan_add(float& s, float& c, float x) {
  const float y = x - c;
  const float t = s + y;
  c = (t - s) - y;
  s = t;
}

template <typename T, bool kPair>
__global__ void gatv2_fwd_kernel(
    const T* __restrict__ hr,             // [Nt.., H, C]
    const T* __restrict__ hl,             // [Ns, H, C]
    const float* __restrict__ att,        // [H, C]
    const int64_t* __restrict__ src,      // [E]
    const int64_t* __restrict__ offsets,  // [Nt+1]
    int64_t n_tgt, int64_t H, int C, float slope, float slope_lo,
    T* __restrict__ out,                  // [Nt, H, C]
    float* __restrict__ m_out,            // [Nt, H]
    float* __restrict__ z_out,            // [Nt, H]
    float* __restrict__ out_f32) {        // [Nt, H, C] unrounded, or null
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t total = n_tgt * H;
  for (int64_t w = wave; w < total; w += n_waves) {
    const int64_t t = w / H;
    const int64_t h = w - t * H;
    const int64_t s0 = offsets[t], s1 = offsets[t + 1];
    float a0, a1, r0, r1;
    row_load<float, kPair>(att + h * C, lane, C, a0, a1);
    row_load<T, kPair>(hr + (t * H + h) * C, lane, C, r0, r1);
    float m = -1e30f, ml = 0.f, Z = 0.f, zc = 0.f;  // max = m + ml
    float acc0 = 0.f, acc1 = 0.f, c0 = 0.f, c1 = 0.f;
    // the online-softmax chain is serial, the row loads of 4 edges overlap
    for (int64_t e = s0; e < s1; e += kEb) {
      const int nb = (int)((s1 - e) < kEb ? (s1 - e) : kEb);
      int64_t sn[kEb];
      float hh0[kEb], hh1[kEb];
      ff sc[kEb];
#pragma unroll
      for (int q = 0; q < kEb; ++q) sn[q] = q < nb ? src[e + q] : sn[0];
#pragma unroll
      for (int q = 0; q < kEb; ++q)
        row_load<T, kPair>(hl + (sn[q] * H + h) * C, lane, C, hh0[q], hh1[q]);
#pragma unroll
      for (int q = 0; q < kEb; ++q)
        sc[q] = score_part(hh0[q], hh1[q], r0, r1, a0, a1, slope, slope_lo);
#pragma unroll
      for (int sft = kWave / 2; sft > 0; sft >>= 1) {
#pragma unroll
        for (int q = 0; q < kEb; ++q) ff_shfl_add(sc[q], sft);
      }
#pragma unroll
      for (int q = 0; q < kEb; ++q) {
        if (q >= nb) continue;
        const ff sv = ff_bcast(sc[q]);
        float p;
        if (sv.h > m || (sv.h == m && sv.l > ml)) {  // wave-uniform
          const float scale = expf((m - sv.h) + (ml - sv.l));
          p = 1.f;
          m = sv.h;
          ml = sv.l;
          Z *= scale;
          zc *= scale;
          acc0 *= scale;
          c0 *= scale;
          acc1 *= scale;
          c1 *= scale;
        } else {
          p = expf((sv.h - m) + (sv.l - ml));
        }
        kahan_add(Z, zc, p);
        kahan_add(acc0, c0, p * hh0[q]);
        kahan_add(acc1, c1, p * hh1[q]);
      }
    }
    const float inv = Z > 0.f ? 1.f / Z : 0.f;
    row_store<T, kPair>(out + (t * H + h) * C, lane, C, acc0 * inv,
                        acc1 * inv);
    if (out_f32 != nullptr)
      row_store<float, kPair>(out_f32 + (t * H + h) * C, lane, C, acc0 * inv,
                              acc1 * inv);
    if (lane == 0) {
      // saved relative to m alone: Z = sum_e exp(score_e - m)
      m_out[t * H + h] = m;
      z_out[t * H + h] = Z * expf(ml);
    }
  }
}

// Backward by target.  nw (a multiple of H) waves work; wave g keeps head
// g % H and takes targets g / H, g / H + nw / H, ...
template <typename T, bool kPair>
__global__ void gatv2_bwd_tgt_kernel(
    const T* __restrict__ hr, const T* __restrict__ hl,
    const float* __restrict__ att, const int64_t* __restrict__ src,
    const int64_t* __restrict__ offsets,
    const float* __restrict__ out,  // [Nt, H, C] the forward's fp32 out
    const float* __restrict__ m_in, const float* __restrict__ z_in,
    const T* __restrict__ dout, int64_t n_tgt, int64_t H, int C, float slope,
    float slope_lo, int64_t nw,
    T* __restrict__ dhr,            // [Nt, H, C]
    float* __restrict__ p_out,      // [E, H] or null (dhl not wanted)
    float* __restrict__ ds_out,     // [E, H] or null: ds before the shift
    float* __restrict__ shift_out,  // [Nt, H] or null
    float* __restrict__ slab) {     // [nw, C] datt partials
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t g = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  if (g >= nw) return;
  const int64_t h = g % H;
  const int64_t t_step = nw / H;
  float a0, a1;
  row_load<float, kPair>(att + h * C, lane, C, a0, a1);
  float da0 = 0.f, da1 = 0.f;
  for (int64_t t = g / H; t < n_tgt; t += t_step) {
    const int64_t s0 = offsets[t], s1 = offsets[t + 1];
    const int64_t row = (t * H + h) * C;
    float g0 = 0.f, g1 = 0.f;  // dhr[t, h, :]
    if (s1 > s0) {
      // ds_e = p_e * (dh_e - D), D = sum_e p_e dh_e = <dout_t, out_t>.  The
      // sweep centres on dot_o, the forward's rounded D, and sums next to
      // every ds-weighted sum X its p-weighted twin Xp; afterwards
      // shift = (sum ds) / (sum p) moves each to X - shift * Xp, which is
      // the sum with D taken from this sweep's own p_e: sum_e ds_e = 0
      // holds to rounding, and the forward's error in out is not
      // multiplied by att into dhr, dhl and datt.
      float gp0 = 0.f, gp1 = 0.f, ta0 = 0.f, ta1 = 0.f, tp0 = 0.f, tp1 = 0.f;
      float ds_sum = 0.f, p_sum = 0.f;
      float r0, r1, d0, d1, o0, o1;
      row_load<T, kPair>(hr + row, lane, C, r0, r1);
      row_load<T, kPair>(dout + row, lane, C, d0, d1);
      row_load<float, kPair>(out + row, lane, C, o0, o1);
      const float dot_o = wave_sum(d0 * o0 + d1 * o1);
      const float m = m_in[t * H + h];
      const float Z = z_in[t * H + h];
      const float inv = Z > 0.f ? 1.f / Z : 0.f;
      for (int64_t e = s0; e < s1; e += kEb) {
        const int nb = (int)((s1 - e) < kEb ? (s1 - e) : kEb);
        int64_t sn[kEb];
        float hh0[kEb], hh1[kEb], dh[kEb];
        ff sc[kEb];
#pragma unroll
        for (int q = 0; q < kEb; ++q) sn[q] = q < nb ? src[e + q] : sn[0];
#pragma unroll
        for (int q = 0; q < kEb; ++q)
          row_load<T, kPair>(hl + (sn[q] * H + h) * C, lane, C, hh0[q],
                             hh1[q]);
#pragma unroll
        for (int q = 0; q < kEb; ++q) {
          sc[q] = score_part(hh0[q], hh1[q], r0, r1, a0, a1, slope,
                             slope_lo);
          dh[q] = hh0[q] * d0 + hh1[q] * d1;
        }
        // 4 score chains (pairs) and 4 dot chains, interleaved
#pragma unroll
        for (int sft = kWave / 2; sft > 0; sft >>= 1) {
#pragma unroll
          for (int q = 0; q < kEb; ++q) {
            ff_shfl_add(sc[q], sft);
            dh[q] += __shfl_down(dh[q], sft);
          }
        }
#pragma unroll
        for (int q = 0; q < kEb; ++q) {
          if (q >= nb) continue;
          const ff sv = ff_bcast(sc[q]);
          const float p = expf((sv.h - m) + sv.l) * inv;
          const float ds = p * (__shfl(dh[q], 0) - dot_o);
          if (p_out != nullptr && lane == 0) {
            p_out[(e + q) * H + h] = p;
            ds_out[(e + q) * H + h] = ds;
          }
          const float u0 = hh0[q] + r0, u1 = hh1[q] + r1;
          const float w0 = a0 * (u0 > 0.f ? 1.f : slope);
          const float w1 = a1 * (u1 > 0.f ? 1.f : slope);
          const float l0 = leaky(u0, slope), l1 = leaky(u1, slope);
          g0 += ds * w0;
          g1 += ds * w1;
          gp0 += p * w0;
          gp1 += p * w1;
          ta0 += ds * l0;
          ta1 += ds * l1;
          tp0 += p * l0;
          tp1 += p * l1;
          ds_sum += ds;
          p_sum += p;
        }
      }
      const float shift = p_sum > 0.f ? ds_sum / p_sum : 0.f;
      g0 -= shift * gp0;
      g1 -= shift * gp1;
      da0 += ta0 - shift * tp0;
      da1 += ta1 - shift * tp1;
      if (shift_out != nullptr && lane == 0) shift_out[t * H + h] = shift;
    }
    row_store<T, kPair>(dhr + row, lane, C, g0, g1);
  }
  row_store<float, kPair>(slab + g * C, lane, C, da0, da1);
}

// Backward by source: dhl[s, h, :] from the in-edge list of s.  kHalf (kPair
// and C <= 64, where a row fills at most 32 lanes): each half of a wave
// takes a (source, head) of its own.  Nothing here crosses lanes, so the
// halves just run their own trip counts; with one or two in-edges per
// source the pass is a chain of dependent loads per wave, and half as many
// waves walk it.
template <typename T, bool kPair, bool kHalf>
__global__ void gatv2_bwd_src_kernel(
    const T* __restrict__ hr, const T* __restrict__ hl,
    const float* __restrict__ att, const int64_t* __restrict__ tgt,
    const int64_t* __restrict__ src_off,  // [Ns+1]
    const int64_t* __restrict__ in_edge,  // [E] edge ids grouped by source
    const float* __restrict__ p_in, const float* __restrict__ ds_in,
    const float* __restrict__ shift_in,   // [Nt, H]
    const T* __restrict__ dout, int64_t n_src, int64_t H, int C, float slope,
    T* __restrict__ dhl) {                // [Ns, H, C]
  static_assert(kPair || !kHalf, "half waves need the paired lane layout");
  constexpr int kLanes = kHalf ? kWave / 2 : kWave;  // lanes per item
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t first =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kLanes;
  const int64_t step = ((int64_t)gridDim.x * blockDim.x) / kLanes;
  const int64_t total = n_src * H;
  for (int64_t w = first; w < total; w += step) {
    const int64_t s = w / H;
    const int64_t h = w - s * H;
    const int64_t i0 = src_off[s], i1 = src_off[s + 1];
    float acc0 = 0.f, acc1 = 0.f;
    if (i1 > i0) {
      float a0, a1, l0, l1;
      row_load<float, kPair>(att + h * C, lane, C, a0, a1);
      row_load<T, kPair>(hl + w * C, lane, C, l0, l1);
      for (int64_t i = i0; i < i1; i += kEb) {
        const int nb = (int)((i1 - i) < kEb ? (i1 - i) : kEb);
        int64_t ee[kEb], tt[kEb];
        float pp[kEb], dd[kEb], d0[kEb], d1[kEb], r0[kEb], r1[kEb];
#pragma unroll
        for (int q = 0; q < kEb; ++q) ee[q] = q < nb ? in_edge[i + q] : ee[0];
#pragma unroll
        for (int q = 0; q < kEb; ++q) {
          tt[q] = tgt[ee[q]];
          pp[q] = p_in[ee[q] * H + h];
          dd[q] = ds_in[ee[q] * H + h];
        }
#pragma unroll
        for (int q = 0; q < kEb; ++q)
          dd[q] -= pp[q] * shift_in[tt[q] * H + h];
#pragma unroll
        for (int q = 0; q < kEb; ++q) {
          const int64_t row = (tt[q] * H + h) * C;
          row_load<T, kPair>(dout + row, lane, C, d0[q], d1[q]);
          row_load<T, kPair>(hr + row, lane, C, r0[q], r1[q]);
        }
#pragma unroll
        for (int q = 0; q < kEb; ++q) {
          if (q >= nb) continue;
          acc0 += pp[q] * d0[q] +
                  dd[q] * a0 * (l0 + r0[q] > 0.f ? 1.f : slope);
          acc1 += pp[q] * d1[q] +
                  dd[q] * a1 * (l1 + r1[q] > 0.f ? 1.f : slope);
        }
      }
    }
    row_store<T, kPair>(dhl + w * C, lane, C, acc0, acc1);
  }
}

// datt[h, c] = sum over the slab rows j * H + h, in a fixed order: thread
// row r adds rows r, r + 16, ... and the 16 sums meet in a fixed tree.
constexpr int kRedRows = 16, kRedCols = 16;

__global__ void gatv2_datt_reduce_kernel(const float* __restrict__ slab,
                                         int64_t n_part, int64_t H, int C,
                                         float* __restrict__ datt) {
  __shared__ float part[kRedRows][kRedCols];
  const int r = threadIdx.x / kRedCols, cc = threadIdx.x % kRedCols;
  const int64_t h = blockIdx.x;
  const int c = blockIdx.y * kRedCols + cc;
  float acc = 0.f;
  if (c < C)
    for (int64_t j = r; j < n_part; j += kRedRows)
      acc += slab[(j * H + h) * C + c];
  part[r][cc] = acc;
  __syncthreads();
#pragma unroll
  for (int half = kRedRows / 2; half > 0; half >>= 1) {
    if (r < half) part[r][cc] += part[r + half][cc];
    __syncthreads();
  }
  if (r == 0 && c < C) datt[h * C + c] = part[0][cc];
}

int gatv2_grid(int64_t waves_needed) {
  const int waves_per_block = kBlock / kWave;
  return (int)std::min<int64_t>(
      (waves_needed + waves_per_block - 1) / waves_per_block, kMaxBlocks);
}

// (H, C) after validating everything the forward and the backward share.
// Shape and dtype come first, the device last, so a caller's mistake is
// named even where there is no device.
std::pair<int64_t, int64_t> gatv2_check(
    const torch::Tensor& h_tgt, const torch::Tensor& h_src,
    const torch::Tensor& att, const torch::Tensor& src,
    const torch::Tensor& offsets, int64_t n_tgt) {
  TORCH_CHECK(h_src.dim() == 3 && h_tgt.dim() == 3,
              "gatv2: h_tgt and h_src must be [N, H, C]");
  TORCH_CHECK(h_src.scalar_type() == torch::kFloat32 ||
                  h_src.scalar_type() == torch::kBFloat16,
              "gatv2: h must be float32 or bfloat16, got ",
              h_src.scalar_type());
  TORCH_CHECK(h_tgt.scalar_type() == h_src.scalar_type(),
              "gatv2: h_tgt and h_src must have one dtype");
  TORCH_CHECK(att.scalar_type() == torch::kFloat32,
              "gatv2: att must be float32, got ", att.scalar_type());
  TORCH_CHECK(src.scalar_type() == torch::kInt64 &&
                  offsets.scalar_type() == torch::kInt64,
              "gatv2: src and offsets must be int64");
  const int64_t H = h_src.size(1), C = h_src.size(2);
  TORCH_CHECK(C >= 1 && C <= 2 * kWave, "gatv2: needs 1 <= C <= 128, got ",
              C);
  TORCH_CHECK(H >= 1 && H <= 1024, "gatv2: needs 1 <= H <= 1024, got ", H);
  TORCH_CHECK(h_tgt.size(1) == H && h_tgt.size(2) == C,
              "gatv2: h_tgt and h_src must agree on [H, C]");
  TORCH_CHECK(att.dim() == 2 && att.size(0) == H && att.size(1) == C,
              "gatv2: att must be [H, C]");
  TORCH_CHECK(src.dim() == 1 && offsets.dim() == 1,
              "gatv2: src and offsets must be 1-D");
  TORCH_CHECK(n_tgt >= 0 && offsets.numel() == n_tgt + 1,
              "gatv2: offsets must have n_tgt + 1 = ", n_tgt + 1,
              " entries, got ", offsets.numel());
  TORCH_CHECK(h_tgt.size(0) >= n_tgt, "gatv2: h_tgt must cover all targets");
  TORCH_CHECK(h_tgt.is_contiguous() && h_src.is_contiguous() &&
                  att.is_contiguous() && src.is_contiguous() &&
                  offsets.is_contiguous(),
              "gatv2: inputs must be contiguous");
  TORCH_CHECK(h_src.is_cuda(), "gatv2: inputs must be on the GPU");
  for (const torch::Tensor* x : {&h_tgt, &att, &src, &offsets})
    TORCH_CHECK(x->device() == h_src.device(),
                "gatv2: inputs must be on one device");
  return {H, C};
}

// two-element row alignment of every tensor the kernels read as rows
bool gatv2_pair(int64_t C, std::initializer_list<const torch::Tensor*> ts) {
  if (C % 2 != 0) return false;
  for (const torch::Tensor* x : ts)
    if ((uintptr_t)x->data_ptr() % (2 * x->element_size()) != 0) return false;
  return true;
}

template <typename Fn>
void with_half(bool v, Fn&& fn) {
  if (v) fn(std::true_type{});
  else fn(std::false_type{});
}

template <typename Fn>
void gatv2_dispatch(bool bf16, bool pair, Fn&& fn) {
  if (bf16) {
    if (pair) fn(c10::BFloat16{}, std::true_type{});
    else fn(c10::BFloat16{}, std::false_type{});
  } else {
    if (pair) fn(float{}, std::true_type{});
    else fn(float{}, std::false_type{});
  }
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor,
           c10::optional<torch::Tensor>>
hip_gatv2_fwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
              const torch::Tensor& att, const torch::Tensor& src,
              const torch::Tensor& offsets, int64_t n_tgt, double slope,
              bool for_backward) {
  const auto hc = gatv2_check(h_tgt, h_src, att, src, offsets, n_tgt);
  const int64_t H = hc.first, C = hc.second;
  auto fopt = h_src.options().dtype(torch::kFloat32);
  const bool bf16 = h_src.scalar_type() == torch::kBFloat16;
  c10::optional<torch::Tensor> out_f32;  // what the backward reads as out
  if (n_tgt == 0 || src.numel() == 0) {
    auto out = torch::zeros({n_tgt, H, C}, h_src.options());
    if (for_backward) out_f32 = bf16 ? torch::zeros({n_tgt, H, C}, fopt) : out;
    return {out, torch::zeros({n_tgt, H}, fopt),
            torch::zeros({n_tgt, H}, fopt), out_f32};
  }
  auto out = torch::empty({n_tgt, H, C}, h_src.options());
  if (for_backward) out_f32 = bf16 ? torch::empty({n_tgt, H, C}, fopt) : out;
  float* accp = bf16 && for_backward ? out_f32->data_ptr<float>() : nullptr;
  auto m = torch::empty({n_tgt, H}, fopt);
  auto z = torch::empty({n_tgt, H}, fopt);
  const bool pair = gatv2_pair(C, {&h_tgt, &h_src, &att, &out});
  const int C_ = (int)C;
  const float slope_hi = (float)slope;
  const float slope_lo = (float)(slope - (double)slope_hi);
  gatv2_dispatch(
      bf16, pair, [&](auto tag, auto kp) {
        using T = decltype(tag);
        hipLaunchKernelGGL((gatv2_fwd_kernel<T, decltype(kp)::value>),
                           dim3(gatv2_grid(n_tgt * H)), dim3(kBlock), 0,
                           current_stream(),
                           reinterpret_cast<const T*>(h_tgt.data_ptr()),
                           reinterpret_cast<const T*>(h_src.data_ptr()),
                           att.data_ptr<float>(), src.data_ptr<int64_t>(),
                           offsets.data_ptr<int64_t>(), n_tgt, H, C_,
                           slope_hi, slope_lo,
                           reinterpret_cast<T*>(out.data_ptr()),
                           m.data_ptr<float>(), z.data_ptr<float>(), accp);
      });
  return {out, m, z, out_f32};
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>, torch::Tensor>
hip_gatv2_bwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
              const torch::Tensor& att, const torch::Tensor& tgt,
              const torch::Tensor& src, const torch::Tensor& offsets,
              const torch::Tensor& out, const torch::Tensor& m,
              const torch::Tensor& z, const torch::Tensor& dout,
              double slope, const c10::optional<torch::Tensor>& src_off,
              const c10::optional<torch::Tensor>& in_edge) {
  const int64_t n_tgt = offsets.numel() - 1;
  const auto hc = gatv2_check(h_tgt, h_src, att, src, offsets, n_tgt);
  const int64_t H = hc.first, C = hc.second;
  const int64_t E = src.numel(), n_src = h_src.size(0);
  const bool need_dhl = src_off.has_value();
  auto is_f32 = [&](const torch::Tensor& x, int64_t n) {
    return x.scalar_type() == torch::kFloat32 && x.is_contiguous() &&
           x.numel() == n && x.device() == h_src.device();
  };
  auto is_idx = [&](const torch::Tensor& x, int64_t n) {
    return x.scalar_type() == torch::kInt64 && x.is_contiguous() &&
           x.dim() == 1 && x.numel() == n && x.device() == h_src.device();
  };
  for (const torch::Tensor* x : {&out, &dout})
    TORCH_CHECK(x->dim() == 3 && x->size(0) == n_tgt && x->size(1) == H &&
                    x->size(2) == C && x->is_contiguous() &&
                    x->device() == h_src.device(),
                "gatv2_bwd: out and dout must be contiguous [n_tgt, H, C] "
                "tensors on h's device");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 &&
                  dout.scalar_type() == h_src.scalar_type(),
              "gatv2_bwd: out must be the forward's float32 out and dout of "
              "h's dtype");
  TORCH_CHECK(is_f32(m, n_tgt * H) && is_f32(z, n_tgt * H),
              "gatv2_bwd: m and Z must be contiguous float32 [n_tgt, H]");
  TORCH_CHECK(is_idx(tgt, E), "gatv2_bwd: tgt must be int64 [E] on device");
  TORCH_CHECK(need_dhl == in_edge.has_value(),
              "gatv2_bwd: src_off and in_edge come together");
  if (need_dhl)
    TORCH_CHECK(is_idx(*src_off, n_src + 1) && is_idx(*in_edge, E),
                "gatv2_bwd: src_off must be int64 [n_src + 1] and in_edge "
                "int64 [E] (segment_transpose(src, n_src, None))");
  auto fopt = h_src.options().dtype(torch::kFloat32);
  c10::optional<torch::Tensor> dhl;
  if (n_tgt == 0 || E == 0) {
    if (need_dhl) dhl = torch::zeros(h_src.sizes(), h_src.options());
    return {torch::zeros(h_tgt.sizes(), h_tgt.options()), dhl,
            torch::zeros({H, C}, fopt)};
  }
  // the kernel writes rows [0, n_tgt) of dhr; rows past them take no edge
  auto dhr = torch::empty(h_tgt.sizes(), h_tgt.options());
  if (h_tgt.size(0) > n_tgt)
    dhr.narrow(0, n_tgt, h_tgt.size(0) - n_tgt).zero_();
  torch::Tensor p, ds, shift;
  if (need_dhl) {
    p = torch::empty({E, H}, fopt);
    ds = torch::empty({E, H}, fopt);
    // rows of targets without edges are never read: no source lists them
    shift = torch::empty({n_tgt, H}, fopt);
    dhl = torch::empty(h_src.sizes(), h_src.options());
  }
  const int blocks = gatv2_grid(n_tgt * H);
  const int64_t nw = ((int64_t)blocks * (kBlock / kWave) / H) * H;
  auto slab = torch::empty({nw, C}, fopt);
  auto datt = torch::empty({H, C}, fopt);
  const bool pair = need_dhl
      ? gatv2_pair(C, {&h_tgt, &h_src, &att, &out, &dout, &dhr, &slab, &*dhl})
      : gatv2_pair(C, {&h_tgt, &h_src, &att, &out, &dout, &dhr, &slab});
  const int C_ = (int)C;
  const float slope_hi = (float)slope;
  const float slope_lo = (float)(slope - (double)slope_hi);
  hipStream_t stream = current_stream();
  gatv2_dispatch(
      h_src.scalar_type() == torch::kBFloat16, pair, [&](auto tag, auto kp) {
        using T = decltype(tag);
        constexpr bool kPair = decltype(kp)::value;
        hipLaunchKernelGGL(
            (gatv2_bwd_tgt_kernel<T, kPair>), dim3(blocks), dim3(kBlock), 0,
            stream, reinterpret_cast<const T*>(h_tgt.data_ptr()),
            reinterpret_cast<const T*>(h_src.data_ptr()),
            att.data_ptr<float>(), src.data_ptr<int64_t>(),
            offsets.data_ptr<int64_t>(),
            out.data_ptr<float>(), m.data_ptr<float>(),
            z.data_ptr<float>(), reinterpret_cast<const T*>(dout.data_ptr()),
            n_tgt, H, C_, slope_hi, slope_lo, nw,
            reinterpret_cast<T*>(dhr.data_ptr()),
            need_dhl ? p.data_ptr<float>() : nullptr,
            need_dhl ? ds.data_ptr<float>() : nullptr,
            need_dhl ? shift.data_ptr<float>() : nullptr,
            slab.data_ptr<float>());
        if (need_dhl)
          with_half(kPair && C <= kWave, [&](auto kh) {
            constexpr bool kHalf = kPair && decltype(kh)::value;
            hipLaunchKernelGGL(
                (gatv2_bwd_src_kernel<T, kPair, kHalf>),
                dim3(gatv2_grid((n_src * H + (kHalf ? 1 : 0)) /
                                (kHalf ? 2 : 1))),
                dim3(kBlock), 0, stream,
                reinterpret_cast<const T*>(h_tgt.data_ptr()),
                reinterpret_cast<const T*>(h_src.data_ptr()),
                att.data_ptr<float>(), tgt.data_ptr<int64_t>(),
                src_off->data_ptr<int64_t>(), in_edge->data_ptr<int64_t>(),
                p.data_ptr<float>(), ds.data_ptr<float>(),
                shift.data_ptr<float>(),
                reinterpret_cast<const T*>(dout.data_ptr()), n_src, H, C_,
                (float)slope, reinterpret_cast<T*>(dhl->data_ptr()));
          });
      });
  hipLaunchKernelGGL(gatv2_datt_reduce_kernel,
                     dim3((unsigned)H,
                          (unsigned)((C + kRedCols - 1) / kRedCols)),
                     dim3(kRedRows * kRedCols), 0, stream,
                     slab.data_ptr<float>(), nw / H, H, C_,
                     datt.data_ptr<float>());
  return {dhr, dhl, datt};
}

}  // namespace glt

/* Fused dot-product graph attention with edge features (PyG's
 * TransformerConv, the UniMP layer) for gfx950, forward and an atomic-free
 * backward.
 *
 * Edges sorted by target, t = tgt[e], s = src[e]; q [Nt.., H, C],
 * k, v [Ns, H, C], optional ee [E, H, C] (projected edge features):
 *
 *   kk_e       = k[s] + ee[e],  vv_e = v[s] + ee[e]
 *   score_e[h] = scale * <q[t,h,:], kk_e[h,:]>
 *   p_e[h]     = softmax over seg(t) of score_e[h]
 *   out[t,h,:] = sum_{e in seg(t)} p_e[h] * vv_e[h,:]     (empty segment: 0)
 *
 *   ds_e   = p_e * (<dout_t, vv_e> - <dout_t, out_t>)
 *   dq[t]  = scale * sum_{e in seg(t)} ds_e * kk_e
 *   dk[s]  = scale * sum_{e: src[e]=s} ds_e * q[t_e]
 *   dv[s]  =         sum_{e: src[e]=s} p_e * dout[t_e]
 *   dee[e] = scale * ds_e * q[t] + p_e * dout[t]
 *
 * Lane layouts.  A target's H*C channels are one flat row.
 *   quad (C % 4 == 0, C / 4 a power of two, everything aligned to four
 *     elements): a lane owns 4 consecutive channels, one 8-byte (bf16) or
 *     16-byte (fp32) access; a head is a group of G = C / 4 adjacent lanes
 *     and its dot product an xor butterfly over log2(G) levels that leaves
 *     the score in every lane of the group.  A wave covers 256 channels,
 *     64 / G whole heads: at H = 4, C = 64 one wave serves one target with
 *     all heads and each k, v or ee row of an edge is one wave-wide load.
 *     H*C > 256 takes several waves per target, H*C < 256 idles lanes.
 *   row (any other C <= 128, unaligned views): one wave per (target, head),
 *     channels lane and 64 + lane by scalar accesses, the butterfly runs
 *     over the whole wave.
 * m, Z, p and ds are therefore per-lane values (one per head group), and
 * the online softmax is branch-free.
 *
 * Forward: q[t] in registers, row loads of 4 edges issued together, their
 * reductions interleaved, online softmax with Kahan sums.  Saves (m, Z) and,
 * for bf16 inputs that will be differentiated, the unrounded fp32 out (the
 * reason is the one given in hip_gatv2.hip).  Nothing per edge.
 *
 * Backward, no float atomics:
 *   by target (forward's layout): recomputes score_e with the forward's
 *     code, sums dq[t] in registers, stores p_e and ds_e to [E, H] fp32
 *     scratch.  ds_e is centred on the forward's <dout_t, out_t>; the
 *     p-weighted twin of the dq sum and shift = sum(ds) / sum(p) move it to
 *     the centre this sweep's own p_e give (as in hip_gatv2.hip), so that
 *     sum_e ds_e = 0 holds to rounding.  dee[e] needs the shifted ds_e per
 *     edge, so when dee is wanted a second sweep over the segment (rows
 *     still in cache) recomputes p_e, ds_e and stores the dee rows.
 *   by source, over hip_segment_transpose(src): per source row sums dk and
 *     dv in list order and stores every row once.  Nothing crosses lanes,
 *     so it takes the quad layout for every C % 4 == 0.
 * Every sum has a fixed order: all results are run-to-run identical.
 */
#include "hip_common.h"
#include "../include/common.h"

// No packed fp32 arithmetic in this file's device code.  hip_wave.h is
// included inside the pragma so that its helpers carry the same features
// and inline; nothing below calls a runtime-header function that is not
// forced inline (no __shfl*, no c10 conversions).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "hip_wave.h"

// the Kahan sums below must keep their rounded products
#pragma clang fp contract(off)

namespace glt {

namespace {

constexpr int kTb = 4;            // edges per load batch
constexpr int kQuadItem = 256;    // channels per wave, quad layout
constexpr int kRowItem = 2 * kWave;

__device__ __forceinline__ void kahan(float& s, float& c, float x) {
  const float y = x - c;
  const float t = s + y;
  c = (t - s) - y;
  s = t;
}

__device__ __forceinline__ float dot4(const float (&a)[4],
                                      const float (&b)[4]) {
  return __builtin_fmaf(
      a[3], b[3],
      __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])));
}

// Where a wave's item lies: (target, block) -> first channel, channel count,
// lanes per head, this lane's head (clamped into range for idle lanes).
template <bool kQuad>
struct Item {
  int64_t base;
  int n, G;
  int64_t head;
  bool lead;  // the lane that stores its head's m, Z, p, ds
  __device__ __forceinline__ Item(int64_t b, int lane, int64_t H, int C) {
    if constexpr (kQuad) {
      const int64_t HC = H * C;
      base = b * kQuadItem;
      n = (int)(HC - base < kQuadItem ? HC - base : kQuadItem);
      G = C / 4;
      const bool on = 4 * lane < n;
      head = on ? (base + 4 * lane) / C : 0;
      lead = on && (lane & (G - 1)) == 0;
    } else {
      base = b * C;
      n = C;
      G = kWave;
      head = b;
      lead = lane == 0;
    }
  }
};

template <bool kQuad>
__device__ __forceinline__ int64_t items_per_row(int64_t H, int C) {
  return kQuad ? (H * C + kQuadItem - 1) / kQuadItem : H;
}

__device__ __forceinline__ int wave_index() {
  return __builtin_amdgcn_readfirstlane(
      (int)((blockIdx.x * blockDim.x + threadIdx.x) / kWave));
}

// kk and vv rows of a batch of edges e .. e + nb - 1; slots past nb re-read
// the first row (their terms are dropped by the caller).
template <typename T, bool kQuad>
__device__ __forceinline__ void load_batch(
    const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ ee, const int64_t* __restrict__ src, int64_t e,
    int nb, int64_t ldk, int64_t ldv, int64_t HC, const Item<kQuad>& it,
    int lane, float (&kk)[kTb][4], float (&vv)[kTb][4]) {
  int64_t sn[kTb], en[kTb];
#pragma unroll
  for (int j = 0; j < kTb; ++j) {
    en[j] = j < nb ? e + j : e;
    sn[j] = src[en[j]];
  }
#pragma unroll
  for (int j = 0; j < kTb; ++j) {
    item_load<T, kQuad>(k + sn[j] * ldk + it.base, lane, it.n, kk[j]);
    item_load<T, kQuad>(v + sn[j] * ldv + it.base, lane, it.n, vv[j]);
  }
  if (ee != nullptr) {
    float w[kTb][4];
#pragma unroll
    for (int j = 0; j < kTb; ++j)
      item_load<T, kQuad>(ee + en[j] * HC + it.base, lane, it.n, w[j]);
#pragma unroll
    for (int j = 0; j < kTb; ++j) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kk[j][c] += w[j][c];
        vv[j][c] += w[j][c];
      }
    }
  }
}

template <typename T, bool kQuad>
__global__ void tconv_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ ee,             // [E, H, C] or null
    const int64_t* __restrict__ src,      // [E]
    const int64_t* __restrict__ offsets,  // [Nt+1]
    int64_t n_tgt, int64_t H, int C, int64_t ldq, int64_t ldk, int64_t ldv,
    float scale,
    T* __restrict__ out,                  // [Nt, H, C]
    float* __restrict__ m_out,            // [Nt, H]
    float* __restrict__ z_out,            // [Nt, H]
    float* __restrict__ out_f32) {        // [Nt, H, C] unrounded, or null
  const int lane = threadIdx.x & (kWave - 1);
  const int n_waves = (int)(gridDim.x * blockDim.x / kWave);
  const int64_t HC = H * C;
  const int64_t per_row = items_per_row<kQuad>(H, C);
  const int64_t total = n_tgt * per_row;
  for (int64_t w = wave_index(); w < total; w += n_waves) {
    const int64_t t = w / per_row;
    const Item<kQuad> it(w - t * per_row, lane, H, C);
    const int64_t s0 = offsets[t], s1 = offsets[t + 1];
    float qv[4];
    item_load<T, kQuad>(q + t * ldq + it.base, lane, it.n, qv);
    float m = -1e30f, Z = 0.f, zc = 0.f;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, cc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t e = s0; e < s1; e += kTb) {
      const int nb = (int)((s1 - e) < kTb ? (s1 - e) : kTb);
      float kk[kTb][4], vv[kTb][4], sc[kTb];
      load_batch<T, kQuad>(k, v, ee, src, e, nb, ldk, ldv, HC, it, lane, kk,
                           vv);
#pragma unroll
      for (int j = 0; j < kTb; ++j) sc[j] = dot4(qv, kk[j]);
      group_sum<kTb>(sc, lane, it.G);
#pragma unroll
      for (int j = 0; j < kTb; ++j) {
        if (j >= nb) continue;
        // branch-free online softmax: the lanes of a wave hold several heads
        const float s = sc[j] * scale;
        const float mn = fmaxf(m, s);
        const float r = expf(m - mn), p = expf(s - mn);
        m = mn;
        Z *= r;
        zc *= r;
        kahan(Z, zc, p);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          acc[c] *= r;
          cc[c] *= r;
          kahan(acc[c], cc[c], p * vv[j][c]);
        }
      }
    }
    const float inv = Z > 0.f ? 1.f / Z : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] *= inv;
    item_store<T, kQuad>(out + t * HC + it.base, lane, it.n, acc);
    if (out_f32 != nullptr)
      item_store<float, kQuad>(out_f32 + t * HC + it.base, lane, it.n, acc);
    if (it.lead) {
      m_out[t * H + it.head] = m;
      z_out[t * H + it.head] = Z;
    }
  }
}

template <typename T, bool kQuad>
__global__ void tconv_bwd_tgt_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ ee, const int64_t* __restrict__ src,
    const int64_t* __restrict__ offsets,
    const float* __restrict__ out,  // [Nt, H, C] the forward's fp32 out
    const float* __restrict__ m_in, const float* __restrict__ z_in,
    const T* __restrict__ dout,     // [Nt, H, C]
    int64_t n_tgt, int64_t H, int C, int64_t ldq, int64_t ldk, int64_t ldv,
    float scale,
    T* __restrict__ dq,             // [Nt.., H, C] or null
    float* __restrict__ p_out,      // [E, H] or null (dk, dv not wanted)
    float* __restrict__ ds_out,     // [E, H] or null: ds before the shift
    float* __restrict__ shift_out,  // [Nt, H] or null
    T* __restrict__ dee) {          // [E, H, C] or null
  const int lane = threadIdx.x & (kWave - 1);
  const int n_waves = (int)(gridDim.x * blockDim.x / kWave);
  const int64_t HC = H * C;
  const int64_t per_row = items_per_row<kQuad>(H, C);
  const int64_t total = n_tgt * per_row;
  const int n_pass = dee != nullptr ? 2 : 1;
  for (int64_t w = wave_index(); w < total; w += n_waves) {
    const int64_t t = w / per_row;
    const Item<kQuad> it(w - t * per_row, lane, H, C);
    const int64_t s0 = offsets[t], s1 = offsets[t + 1];
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (s1 > s0) {
      float qv[4], dv[4], ov[4];
      item_load<T, kQuad>(q + t * ldq + it.base, lane, it.n, qv);
      item_load<T, kQuad>(dout + t * HC + it.base, lane, it.n, dv);
      item_load<float, kQuad>(out + t * HC + it.base, lane, it.n, ov);
      float dot_o[1] = {dot4(dv, ov)};
      group_sum<1>(dot_o, lane, it.G);
      const float m = m_in[t * H + it.head];
      const float Z = z_in[t * H + it.head];
      const float inv = Z > 0.f ? 1.f / Z : 0.f;
      float gp[4] = {0.f, 0.f, 0.f, 0.f};
      float ds_sum = 0.f, p_sum = 0.f, shift = 0.f;
      for (int pass = 0; pass < n_pass; ++pass) {
        for (int64_t e = s0; e < s1; e += kTb) {
          const int nb = (int)((s1 - e) < kTb ? (s1 - e) : kTb);
          float kk[kTb][4], vv[kTb][4], red[2 * kTb];
          load_batch<T, kQuad>(k, v, ee, src, e, nb, ldk, ldv, HC, it, lane,
                               kk, vv);
#pragma unroll
          for (int j = 0; j < kTb; ++j) {
            red[j] = dot4(qv, kk[j]);
            red[kTb + j] = dot4(dv, vv[j]);
          }
          // 4 score chains and 4 <dout, vv> chains, interleaved
          group_sum<2 * kTb>(red, lane, it.G);
#pragma unroll
          for (int j = 0; j < kTb; ++j) {
            if (j >= nb) continue;
            const float p = expf(red[j] * scale - m) * inv;
            const float ds = p * (red[kTb + j] - dot_o[0]);
            if (pass == 0) {
              if (p_out != nullptr && it.lead) {
                p_out[(e + j) * H + it.head] = p;
                ds_out[(e + j) * H + it.head] = ds;
              }
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                g[c] += ds * kk[j][c];
                gp[c] += p * kk[j][c];
              }
              ds_sum += ds;
              p_sum += p;
            } else {
              const float dsf = (ds - shift * p) * scale;
              float row[4];
#pragma unroll
              for (int c = 0; c < 4; ++c)
                row[c] = dsf * qv[c] + p * dv[c];
              item_store<T, kQuad>(dee + (e + j) * HC + it.base, lane, it.n,
                                   row);
            }
          }
        }
        if (pass == 0) {
          shift = p_sum > 0.f ? ds_sum / p_sum : 0.f;
          if (shift_out != nullptr && it.lead)
            shift_out[t * H + it.head] = shift;
#pragma unroll
          for (int c = 0; c < 4; ++c) g[c] = (g[c] - shift * gp[c]) * scale;
        }
      }
    }
    if (dq != nullptr)
      item_store<T, kQuad>(dq + t * HC + it.base, lane, it.n, g);
  }
}

// Backward by source: dk[s], dv[s] from the in-edge list of s.  The flat
// [H*C] row is cut into items of 256 (quad) or 128 channels whatever C is;
// a lane looks up p, ds and shift under the head of each of its channels
// (one head per lane in the quad layout, C % 4 == 0).
template <typename T, bool kQuad>
__global__ void tconv_bwd_src_kernel(
    const T* __restrict__ q, const T* __restrict__ dout,
    const int64_t* __restrict__ tgt,
    const int64_t* __restrict__ src_off,  // [Ns+1]
    const int64_t* __restrict__ in_edge,  // [E] edge ids grouped by source
    const float* __restrict__ p_in, const float* __restrict__ ds_in,
    const float* __restrict__ shift_in,   // [Nt, H]
    int64_t n_src, int64_t H, int C, int64_t ldq, float scale,
    T* __restrict__ dk, T* __restrict__ dv) {  // [Ns, H, C]
  constexpr int kItem = kQuad ? kQuadItem : kRowItem;
  constexpr int kNh = kQuad ? 1 : 2;  // heads a lane can touch
  const int lane = threadIdx.x & (kWave - 1);
  const int n_waves = (int)(gridDim.x * blockDim.x / kWave);
  const int64_t HC = H * C;
  const int64_t per_row = (HC + kItem - 1) / kItem;
  const int64_t total = n_src * per_row;
  for (int64_t w = wave_index(); w < total; w += n_waves) {
    const int64_t s = w / per_row;
    const int64_t base = (w - s * per_row) * kItem;
    const int n = (int)(HC - base < kItem ? HC - base : kItem);
    int64_t hd[kNh];
    if constexpr (kQuad) {
      hd[0] = 4 * lane < n ? (base + 4 * lane) / C : 0;
    } else {
      hd[0] = lane < n ? (base + lane) / C : 0;
      hd[1] = kWave + lane < n ? (base + kWave + lane) / C : 0;
    }
    const int64_t i0 = src_off[s], i1 = src_off[s + 1];
    float ak[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = i0; i < i1; i += kTb) {
      const int nb = (int)((i1 - i) < kTb ? (i1 - i) : kTb);
      int64_t ed[kTb], tt[kTb];
      float pp[kTb][kNh], dd[kTb][kNh], qr[kTb][4], dr[kTb][4];
#pragma unroll
      for (int j = 0; j < kTb; ++j) ed[j] = in_edge[j < nb ? i + j : i];
#pragma unroll
      for (int j = 0; j < kTb; ++j) {
        tt[j] = tgt[ed[j]];
#pragma unroll
        for (int x = 0; x < kNh; ++x) {
          pp[j][x] = p_in[ed[j] * H + hd[x]];
          dd[j][x] = ds_in[ed[j] * H + hd[x]];
        }
      }
#pragma unroll
      for (int j = 0; j < kTb; ++j) {
#pragma unroll
        for (int x = 0; x < kNh; ++x)
          dd[j][x] -= pp[j][x] * shift_in[tt[j] * H + hd[x]];
        item_load<T, kQuad>(q + tt[j] * ldq + base, lane, n, qr[j]);
        item_load<T, kQuad>(dout + tt[j] * HC + base, lane, n, dr[j]);
      }
#pragma unroll
      for (int j = 0; j < kTb; ++j) {
        if (j >= nb) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int x = kQuad ? 0 : (c & 1);  // row layout: v[2], v[3] are 0
          ak[c] += dd[j][x] * qr[j][c];
          av[c] += pp[j][x] * dr[j][c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) ak[c] *= scale;
    item_store<T, kQuad>(dk + s * HC + base, lane, n, ak);
    item_store<T, kQuad>(dv + s * HC + base, lane, n, av);
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace {

int tconv_grid(int64_t waves_needed) {
  const int waves_per_block = kBlock / kWave;
  return (int)std::min<int64_t>(
      std::max<int64_t>(
          (waves_needed + waves_per_block - 1) / waves_per_block, 1),
      kMaxBlocks);
}

bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

// base address and row stride on a four-element boundary
bool quad_aligned(const torch::Tensor& x) {
  return (uintptr_t)x.data_ptr() % (4 * x.element_size()) == 0 &&
         (x.dim() < 2 || x.size(0) < 2 || x.stride(0) % 4 == 0);
}

// (H, C) after validating everything the forward and the backward share.
// Shape and dtype come first, the device last, so a caller's mistake is
// named even where there is no device.
std::pair<int64_t, int64_t> tconv_check(
    const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
    const c10::optional<torch::Tensor>& ee, const torch::Tensor& src,
    const torch::Tensor& offsets, int64_t n_tgt) {
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3,
              "tconv: q, k and v must be [N, H, C]");
  TORCH_CHECK(k.scalar_type() == torch::kFloat32 ||
                  k.scalar_type() == torch::kBFloat16,
              "tconv: inputs must be float32 or bfloat16, got ",
              k.scalar_type());
  TORCH_CHECK(q.scalar_type() == k.scalar_type() &&
                  v.scalar_type() == k.scalar_type() &&
                  (!ee.has_value() || ee->scalar_type() == k.scalar_type()),
              "tconv: q, k, v and ee must have one dtype");
  TORCH_CHECK(src.scalar_type() == torch::kInt64 &&
                  offsets.scalar_type() == torch::kInt64,
              "tconv: src and offsets must be int64");
  const int64_t H = k.size(1), C = k.size(2);
  TORCH_CHECK(C >= 1 && C <= 2 * kWave, "tconv: needs 1 <= C <= 128, got ",
              C);
  TORCH_CHECK(H >= 1 && H <= 1024, "tconv: needs 1 <= H <= 1024, got ", H);
  for (const torch::Tensor* x : {&q, &v})
    TORCH_CHECK(x->size(1) == H && x->size(2) == C,
                "tconv: q, k and v must agree on [H, C]");
  TORCH_CHECK(v.size(0) == k.size(0), "tconv: k and v must have n_src rows");
  TORCH_CHECK(src.dim() == 1 && offsets.dim() == 1,
              "tconv: src and offsets must be 1-D");
  TORCH_CHECK(n_tgt >= 0 && offsets.numel() == n_tgt + 1,
              "tconv: offsets must have n_tgt + 1 = ", n_tgt + 1,
              " entries, got ", offsets.numel());
  TORCH_CHECK(q.size(0) >= n_tgt, "tconv: q must cover all targets");
  if (ee.has_value())
    TORCH_CHECK(ee->dim() == 3 && ee->size(0) == src.numel() &&
                    ee->size(1) == H && ee->size(2) == C &&
                    ee->is_contiguous(),
                "tconv: ee must be contiguous [E, H, C] with E = ",
                src.numel(), " rows");
  // rows may be strided (column slices of one projection); [H, C] is dense
  for (const torch::Tensor* x : {&q, &k, &v})
    TORCH_CHECK(x->numel() == 0 ||
                    (x->stride(2) == 1 && x->stride(1) == C &&
                     (x->size(0) < 2 || x->stride(0) >= H * C)),
                "tconv: q, k and v need a contiguous inner [H, C]");
  TORCH_CHECK(src.is_contiguous() && offsets.is_contiguous(),
              "tconv: src and offsets must be contiguous");
  TORCH_CHECK(k.is_cuda(), "tconv: inputs must be on the GPU");
  for (const torch::Tensor* x : {&q, &v, &src, &offsets})
    TORCH_CHECK(x->device() == k.device(),
                "tconv: inputs must be on one device");
  TORCH_CHECK(!ee.has_value() || ee->device() == k.device(),
              "tconv: inputs must be on one device");
  return {H, C};
}

int64_t row_stride(const torch::Tensor& x) {
  return x.size(0) < 2 ? x.size(1) * x.size(2) : x.stride(0);
}

template <typename Fn>
void tconv_dispatch(bool bf16, bool quad, Fn&& fn) {
  if (bf16) {
    if (quad) fn(c10::BFloat16{}, std::true_type{});
    else fn(c10::BFloat16{}, std::false_type{});
  } else {
    if (quad) fn(float{}, std::true_type{});
    else fn(float{}, std::false_type{});
  }
}

template <typename T>
const T* cptr(const torch::Tensor& x) {
  return reinterpret_cast<const T*>(x.data_ptr());
}

template <typename T>
const T* cptr(const c10::optional<torch::Tensor>& x) {
  return x.has_value() ? reinterpret_cast<const T*>(x->data_ptr()) : nullptr;
}

template <typename T>
T* mptr(const c10::optional<torch::Tensor>& x) {
  return x.has_value() ? reinterpret_cast<T*>(x->data_ptr()) : nullptr;
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor,
           c10::optional<torch::Tensor>>
hip_tconv_fwd(const torch::Tensor& q, const torch::Tensor& k,
              const torch::Tensor& v, const c10::optional<torch::Tensor>& ee,
              const torch::Tensor& src, const torch::Tensor& offsets,
              int64_t n_tgt, double scale, bool for_backward) {
  const auto hc = tconv_check(q, k, v, ee, src, offsets, n_tgt);
  const int64_t H = hc.first, C = hc.second;
  auto opt = k.options();
  auto fopt = opt.dtype(torch::kFloat32);
  const bool bf16 = k.scalar_type() == torch::kBFloat16;
  c10::optional<torch::Tensor> out_f32;  // what the backward reads as out
  if (n_tgt == 0 || src.numel() == 0) {
    auto out = torch::zeros({n_tgt, H, C}, opt);
    if (for_backward) out_f32 = bf16 ? torch::zeros({n_tgt, H, C}, fopt) : out;
    return {out, torch::zeros({n_tgt, H}, fopt),
            torch::zeros({n_tgt, H}, fopt), out_f32};
  }
  auto out = torch::empty({n_tgt, H, C}, opt);
  if (for_backward) out_f32 = bf16 ? torch::empty({n_tgt, H, C}, fopt) : out;
  float* accp = bf16 && for_backward ? out_f32->data_ptr<float>() : nullptr;
  auto m = torch::empty({n_tgt, H}, fopt);
  auto z = torch::empty({n_tgt, H}, fopt);
  const bool quad = C % 4 == 0 && is_pow2(C / 4) && quad_aligned(q) &&
                    quad_aligned(k) && quad_aligned(v) &&
                    (!ee.has_value() || quad_aligned(*ee));
  const int64_t per_row = quad ? (H * C + kQuadItem - 1) / kQuadItem : H;
  tconv_dispatch(bf16, quad, [&](auto tag, auto kq) {
    using T = decltype(tag);
    hipLaunchKernelGGL((tconv_fwd_kernel<T, decltype(kq)::value>),
                       dim3(tconv_grid(n_tgt * per_row)), dim3(kBlock), 0,
                       current_stream(), cptr<T>(q), cptr<T>(k), cptr<T>(v),
                       cptr<T>(ee), src.data_ptr<int64_t>(),
                       offsets.data_ptr<int64_t>(), n_tgt, H, (int)C,
                       row_stride(q), row_stride(k), row_stride(v),
                       (float)scale, reinterpret_cast<T*>(out.data_ptr()),
                       m.data_ptr<float>(), z.data_ptr<float>(), accp);
  });
  return {out, m, z, out_f32};
}

std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
hip_tconv_bwd(const torch::Tensor& q, const torch::Tensor& k,
              const torch::Tensor& v, const c10::optional<torch::Tensor>& ee,
              const torch::Tensor& tgt, const torch::Tensor& src,
              const torch::Tensor& offsets, const torch::Tensor& out,
              const torch::Tensor& m, const torch::Tensor& z,
              const torch::Tensor& dout, double scale, bool need_dq,
              bool need_dee, const c10::optional<torch::Tensor>& src_off,
              const c10::optional<torch::Tensor>& in_edge) {
  const int64_t n_tgt = offsets.numel() - 1;
  const auto hc = tconv_check(q, k, v, ee, src, offsets, n_tgt);
  const int64_t H = hc.first, C = hc.second;
  const int64_t E = src.numel(), n_src = k.size(0);
  const bool need_dkv = src_off.has_value();
  auto is_f32 = [&](const torch::Tensor& x, int64_t n) {
    return x.scalar_type() == torch::kFloat32 && x.is_contiguous() &&
           x.numel() == n && x.device() == k.device();
  };
  auto is_idx = [&](const torch::Tensor& x, int64_t n) {
    return x.scalar_type() == torch::kInt64 && x.is_contiguous() &&
           x.dim() == 1 && x.numel() == n && x.device() == k.device();
  };
  for (const torch::Tensor* x : {&out, &dout})
    TORCH_CHECK(x->dim() == 3 && x->size(0) == n_tgt && x->size(1) == H &&
                    x->size(2) == C && x->is_contiguous() &&
                    x->device() == k.device(),
                "tconv_bwd: out and dout must be contiguous [n_tgt, H, C] "
                "tensors on the inputs' device");
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 &&
                  dout.scalar_type() == k.scalar_type(),
              "tconv_bwd: out must be the forward's float32 out and dout of "
              "the inputs' dtype");
  TORCH_CHECK(is_f32(m, n_tgt * H) && is_f32(z, n_tgt * H),
              "tconv_bwd: m and Z must be contiguous float32 [n_tgt, H]");
  TORCH_CHECK(is_idx(tgt, E), "tconv_bwd: tgt must be int64 [E] on device");
  TORCH_CHECK(need_dkv == in_edge.has_value(),
              "tconv_bwd: src_off and in_edge come together");
  TORCH_CHECK(!need_dee || ee.has_value(),
              "tconv_bwd: need_dee without ee");
  if (need_dkv)
    TORCH_CHECK(is_idx(*src_off, n_src + 1) && is_idx(*in_edge, E),
                "tconv_bwd: src_off must be int64 [n_src + 1] and in_edge "
                "int64 [E] (segment_transpose(src, n_src, None))");
  auto opt = k.options();
  auto fopt = opt.dtype(torch::kFloat32);
  c10::optional<torch::Tensor> dq, dk, dv, dee;
  if (n_tgt == 0 || E == 0) {
    if (need_dq) dq = torch::zeros(q.sizes(), opt);
    if (need_dkv) {
      dk = torch::zeros(k.sizes(), opt);
      dv = torch::zeros(v.sizes(), opt);
    }
    if (need_dee) dee = torch::zeros(ee->sizes(), opt);
    return {dq, dk, dv, dee};
  }
  if (need_dq) {
    // the kernel writes rows [0, n_tgt); rows past them take no edge
    dq = torch::empty(q.sizes(), opt);
    if (q.size(0) > n_tgt) dq->narrow(0, n_tgt, q.size(0) - n_tgt).zero_();
  }
  c10::optional<torch::Tensor> p, ds, shift;
  if (need_dkv) {
    p = torch::empty({E, H}, fopt);
    ds = torch::empty({E, H}, fopt);
    // rows of targets without edges are never read: no source lists them
    shift = torch::empty({n_tgt, H}, fopt);
    dk = torch::empty({n_src, H, C}, opt);
    dv = torch::empty({n_src, H, C}, opt);
  }
  if (need_dee) dee = torch::empty({E, H, C}, opt);
  const bool bf16 = k.scalar_type() == torch::kBFloat16;
  hipStream_t stream = current_stream();
  if (need_dq || need_dkv || need_dee) {
    const bool quad = C % 4 == 0 && is_pow2(C / 4) && quad_aligned(q) &&
                      quad_aligned(k) && quad_aligned(v) &&
                      quad_aligned(dout) && quad_aligned(out) &&
                      (!ee.has_value() || quad_aligned(*ee));
    const int64_t per_row = quad ? (H * C + kQuadItem - 1) / kQuadItem : H;
    tconv_dispatch(bf16, quad, [&](auto tag, auto kq) {
      using T = decltype(tag);
      hipLaunchKernelGGL(
          (tconv_bwd_tgt_kernel<T, decltype(kq)::value>),
          dim3(tconv_grid(n_tgt * per_row)), dim3(kBlock), 0, stream,
          cptr<T>(q), cptr<T>(k), cptr<T>(v), cptr<T>(ee),
          src.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
          out.data_ptr<float>(), m.data_ptr<float>(), z.data_ptr<float>(),
          cptr<T>(dout), n_tgt, H, (int)C, row_stride(q), row_stride(k),
          row_stride(v), (float)scale, mptr<T>(dq), mptr<float>(p),
          mptr<float>(ds), mptr<float>(shift), mptr<T>(dee));
    });
  }
  if (need_dkv) {
    const bool quad = C % 4 == 0 && quad_aligned(q) && quad_aligned(dout);
    const int64_t item = quad ? kQuadItem : kRowItem;
    const int64_t per_row = (H * C + item - 1) / item;
    tconv_dispatch(bf16, quad, [&](auto tag, auto kq) {
      using T = decltype(tag);
      hipLaunchKernelGGL(
          (tconv_bwd_src_kernel<T, decltype(kq)::value>),
          dim3(tconv_grid(n_src * per_row)), dim3(kBlock), 0, stream,
          cptr<T>(q), cptr<T>(dout), tgt.data_ptr<int64_t>(),
          src_off->data_ptr<int64_t>(), in_edge->data_ptr<int64_t>(),
          p->data_ptr<float>(), ds->data_ptr<float>(),
          shift->data_ptr<float>(), n_src, H, (int)C, row_stride(q),
          (float)scale, mptr<T>(dk), mptr<T>(dv));
    });
  }
  return {dq, dk, dv, dee};
}

}  // namespace glt

/* Fused GAT edge-softmax + weighted aggregation (gfx950).
 *
 * Replaces the whole torch chain per GATConv — including the per-node
 * attention-logit precompute (h*att).sum(-1) — with one forward and one
 * backward kernel.  The logits are recomputed per edge from rows the
 * aggregation loads anyway (a 6-step wave reduction on data already in
 * registers), which deletes ~8 small launches per relation per layer in
 * RGAT's launch-bound regime.
 *
 * Layout: edges sorted by target (glt_amd batch invariant); one wave per
 * (target, head), lanes over the channel dim; the softmax runs online
 * (running max / rescaled sum) along the target's edge segment, so scores
 * are never materialized.
 *
 *   s_e   = leaky_relu(<h_tgt[t,h,:], att_dst[h,:]> +
 *                      <h_src[src_e,h,:], att_src[h,:]>)
 *   p_e   = exp(s_e - m_t) / Z_t
 *   out_t = sum_e p_e * h_src[src_e,h,:]
 *
 * Backward recomputes s_e from the saved (m, Z) statistics:
 *   dh_src[src_e]  += p_e * dout_t + ds_e * att_src[h]   (fp32 atomics)
 *   ds_e            = p_e * (<dout_t, h_src_e> - <dout_t, out_t>)
 *                     * leaky'(s_pre_e)
 *   datt_src[h]    += ds_e * h_src[src_e];  dh_tgt[t] += (sum ds) * att_dst
 *   datt_dst[h]    += (sum_e ds_e) * h_tgt[t]
 *
 * One device body per direction (gat_fwd_item, gat_bwd_item) works on one
 * relation's view (GatRel); one kernel per direction walks a packed table of
 * up to 8 relations, so a hetero layer is ONE forward and ONE backward
 * launch (RGAT's step is launch-bound).  h rows are addressed base +
 * n*stride + h*C + c, so dh accumulates atomically straight into a per-type
 * arena.  A single GATConv is the one-relation table; its forward runs the
 * body from a thin kernel with __restrict__ arguments (gat_fwd_one_kernel).
 */
#include <hip/hip_bf16.h>

#include "hip_wave.h"
#include "../include/common.h"

namespace glt {

namespace {

constexpr int kMaxRel = 8;

template <typename T>  // h/out dtype: float or bf16 (math stays fp32)
struct GatRel {
  const T* h_tgt;           // [Nt.., H, C], rows tgt_stride apart
  const T* h_src;           // [Ns, H, C], rows src_stride apart
  int64_t tgt_stride, src_stride;
  const float* att_src;     // [H, C]
  const float* att_dst;     // [H, C]
  const int64_t* src;       // [E]
  const int64_t* off;       // [Nt+1]
  T* out;                   // [Nt, H, C] contiguous
  float* m;                 // [Nt, H]
  float* z;                 // [Nt, H]
  float* spre;              // [E, H] pre-activation logits
  const T* dout;            // bwd only, [Nt, H, C] contiguous
  float* dh_tgt;            // bwd only (fp32 arenas, row-strided)
  float* dh_src;
  int64_t dht_stride, dhs_stride;
  float* datt_src;          // bwd only, [H, C]
  float* datt_dst;
  const float* bias;        // fwd: optional [H*C], added to out
};

template <typename T>
struct GatPack {
  GatRel<T> rel[kMaxRel];
  int64_t cum[kMaxRel + 1];  // cumulative n_tgt (work-item decode)
  int n_rel;
};

// The relation that global target tg belongs to.  It is wave-uniform by
// construction (tg comes from the wave index); telling the compiler so keeps
// every P.rel[r] field a scalar load instead of per-lane kernarg fetches.
template <typename T>
__device__ __forceinline__ int gat_rel_of(const GatPack<T>& P, int64_t tg) {
  int r = 0;
  while (r + 1 < P.n_rel && tg >= P.cum[r + 1]) ++r;
  return __builtin_amdgcn_readfirstlane(r);
}

template <typename T>
__device__ __forceinline__ void gat_fwd_item(const GatRel<T>& rel, int64_t t,
                                             int64_t h, int64_t H, int64_t C,
                                             float slope, int lane) {
  const int64_t s0 = rel.off[t], s1 = rel.off[t + 1];
  const float* atd = rel.att_dst + h * C;
  float as0, as1;
  row_load<float, false>(rel.att_src + h * C, lane, (int)C, as0, as1);
  const T* tv = rel.h_tgt + t * rel.tgt_stride + h * C;
  const float ad = wave_sum(
      (lane < C ? (float)tv[lane] * atd[lane] : 0.f) +
      (kWave + lane < C ? (float)tv[kWave + lane] * atd[kWave + lane]
                        : 0.f));
  float m = -1e30f, Z = 0.f;
  float acc0 = 0.f, acc1 = 0.f;  // lanes cover C (up to 2 passes)
  const int64_t hstride = rel.src_stride;
  const T* hbase = rel.h_src + h * C;
  // 4-edge load batching (see backward): the online-softmax chain
  // stays serial but its global loads overlap.
  for (int64_t e = s0; e < s1; e += 4) {
    const int nb = (int)((s1 - e) < 4 ? (s1 - e) : 4);
    int64_t sn[4];
    float hh0[4], hh1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sn[q] = q < nb ? rel.src[e + q] : sn[0];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      row_load<T, false>(hbase + sn[q] * hstride, lane, (int)C, hh0[q],
                         hh1[q]);
    float sc4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sc4[q] = hh0[q] * as0 + hh1[q] * as1;
#pragma unroll
    for (int sft = kWave / 2; sft > 0; sft >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sc4[q] += __shfl_down(sc4[q], sft);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= nb) continue;
      float sv = ad + __shfl(sc4[q], 0);
      if (lane == 0) rel.spre[(e + q) * H + h] = sv;
      sv = sv > 0.f ? sv : sv * slope;
      float scale = 1.f;
      float p;
      if (sv > m) {
        scale = __expf(m - sv);
        p = 1.f;
        m = sv;
      } else {
        p = __expf(sv - m);
      }
      Z = Z * scale + p;
      acc0 = acc0 * scale + p * hh0[q];
      acc1 = acc1 * scale + p * hh1[q];
    }
  }
  const float inv = Z > 0.f ? 1.f / Z : 0.f;
  float o0 = acc0 * inv, o1 = acc1 * inv;
  if (rel.bias) {  // one rounding with a bias, and no "+ 0.f" without one
    float b0, b1;
    row_load<float, false>(rel.bias + h * C, lane, (int)C, b0, b1);
    o0 = __fmaf_rn(acc0, inv, b0);
    o1 = __fmaf_rn(acc1, inv, b1);
  }
  row_store<T, false>(rel.out + (t * H + h) * C, lane, (int)C, o0, o1);
  if (lane == 0) {
    rel.m[t * H + h] = m;
    rel.z[t * H + h] = Z;
  }
}

// S-way segment split: small-target layers (hop 0: 512 targets x 4
// heads = 2048 waves) cannot fill 256 CUs with (t, h) waves alone —
// every per-edge term in the backward is independent given the saved
// (m, Z, out) statistics, so S sub-waves each take a slice of the
// segment and flush their partial reductions atomically.  This is
// sub-wave q of S.
template <typename T>
__device__ __forceinline__ void gat_bwd_item(const GatRel<T>& rel, int64_t t,
                                             int64_t h, int64_t q, int64_t S,
                                             int64_t H, int64_t C,
                                             float slope, int lane) {
  const int64_t f0 = rel.off[t], f1 = rel.off[t + 1];
  if (f1 <= f0) return;
  const int64_t per = (f1 - f0 + S - 1) / S;
  const int64_t s0 = f0 + q * per;
  const int64_t s1 = s0 + per < f1 ? s0 + per : f1;
  if (s1 <= s0) return;
  float as0, as1, t0, t1, ad0, ad1, d0, d1;
  row_load<float, false>(rel.att_src + h * C, lane, (int)C, as0, as1);
  row_load<T, false>(rel.h_tgt + t * rel.tgt_stride + h * C, lane, (int)C,
                     t0, t1);
  row_load<float, false>(rel.att_dst + h * C, lane, (int)C, ad0, ad1);
  const float m = rel.m[t * H + h];
  const float Z = rel.z[t * H + h];
  const float inv = Z > 0.f ? 1.f / Z : 0.f;
  const T* ov = rel.out + (t * H + h) * C;
  row_load<T, false>(rel.dout + (t * H + h) * C, lane, (int)C, d0, d1);
  const float dot_o = wave_sum(
      (lane < C ? d0 * (float)ov[lane] : 0.f) +
      (kWave + lane < C ? d1 * (float)ov[kWave + lane] : 0.f));
  float dad_acc = 0.f;           // sum of ds over the segment
  float das0 = 0.f, das1 = 0.f;  // datt_src accumulator (per lane)
  const int64_t hstride = rel.src_stride;
  const int64_t dstride = rel.dhs_stride;
  const T* hbase = rel.h_src + h * C;
  float* dhbase = rel.dh_src + h * C;
  // 4-edge software pipeline: the segment loop was a serial chain of
  // dependent global loads (src[e] -> h_src row -> math), ~10 L2-miss
  // latencies back to back per wave; batching the loads of 4 edges
  // gives the memory system 4 independent misses in flight and lets
  // the 4 wave-reductions interleave.
  for (int64_t e = s0; e < s1; e += 4) {
    const int nb = (int)((s1 - e) < 4 ? (s1 - e) : 4);
    int64_t sn[4];
    float hh0[4], hh1[4], spre4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sn[q] = q < nb ? rel.src[e + q] : sn[0];
      if (q < nb) spre4[q] = rel.spre[(e + q) * H + h];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      row_load<T, false>(hbase + sn[q] * hstride, lane, (int)C, hh0[q],
                         hh1[q]);
    float dot_h4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) dot_h4[q] = hh0[q] * d0 + hh1[q] * d1;
    // interleaved wave reductions (independent shfl chains)
#pragma unroll
    for (int sft = kWave / 2; sft > 0; sft >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) dot_h4[q] += __shfl_down(dot_h4[q], sft);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= nb) continue;
      const float s_pre = spre4[q];
      const float sa = s_pre > 0.f ? s_pre : s_pre * slope;
      const float p = __expf(sa - m) * inv;
      float ds = p * (__shfl(dot_h4[q], 0) - dot_o);
      ds *= (s_pre > 0.f ? 1.f : slope);
      float* dhv = dhbase + sn[q] * dstride;
      if (lane < C) atomicAdd(&dhv[lane], p * d0 + ds * as0);
      if (kWave + lane < C) atomicAdd(&dhv[kWave + lane], p * d1 + ds * as1);
      das0 += ds * hh0[q];
      das1 += ds * hh1[q];
      dad_acc += ds;
    }
  }
  // one atomic flush per wave (not per edge)
  float* dtv = rel.dh_tgt + t * rel.dht_stride + h * C;
  if (lane < C) {
    atomicAdd(&dtv[lane], dad_acc * ad0);
    atomicAdd(&rel.datt_src[h * C + lane], das0);
    atomicAdd(&rel.datt_dst[h * C + lane], dad_acc * t0);
  }
  if (kWave + lane < C) {
    atomicAdd(&dtv[kWave + lane], dad_acc * ad1);
    atomicAdd(&rel.datt_src[h * C + kWave + lane], das1);
    atomicAdd(&rel.datt_dst[h * C + kWave + lane], dad_acc * t1);
  }
}

template <typename T>
__global__ void gat_fwd_kernel(GatPack<T> P, int64_t H, int64_t C,
                               float slope, int64_t total) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t w = wave; w < total * H; w += n_waves) {
    const int64_t tg = w / H;
    const int64_t h = w - tg * H;
    const int r = gat_rel_of(P, tg);
    gat_fwd_item<T>(P.rel[r], tg - P.cum[r], h, H, C, slope, lane);
  }
}

// One relation, its pointers as __restrict__ kernel arguments: the same body
// on a GatRel filled here.  Through the pack the forward ran 45% longer at
// GATConv's shape (732 against 504 us, profiles/r07_gat_one_body.md); the
// backward did not, and has no such wrapper.
template <typename T>
__global__ void gat_fwd_one_kernel(
    const T* __restrict__ h_tgt, const T* __restrict__ h_src,
    const float* __restrict__ att_src, const float* __restrict__ att_dst,
    const int64_t* __restrict__ src, const int64_t* __restrict__ off,
    int64_t n_tgt, int64_t H, int64_t C, float slope, T* __restrict__ out,
    float* __restrict__ m, float* __restrict__ z, float* __restrict__ spre) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  GatRel<T> rel{};
  rel.h_tgt = h_tgt;
  rel.h_src = h_src;
  rel.tgt_stride = rel.src_stride = H * C;
  rel.att_src = att_src;
  rel.att_dst = att_dst;
  rel.src = src;
  rel.off = off;
  rel.out = out;
  rel.m = m;
  rel.z = z;
  rel.spre = spre;
  for (int64_t w = wave; w < n_tgt * H; w += n_waves) {
    const int64_t t = w / H;
    gat_fwd_item<T>(rel, t, w - t * H, H, C, slope, lane);
  }
}

template <typename T>
__global__ void gat_bwd_kernel(GatPack<T> P, int64_t H, int64_t C,
                               float slope, int64_t S, int64_t total) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave =
      (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
  for (int64_t w = wave; w < total * H * S; w += n_waves) {
    const int64_t tg = w / (H * S);
    const int64_t rem = w - tg * H * S;
    const int64_t h = rem / S;
    const int r = gat_rel_of(P, tg);
    gat_bwd_item<T>(P.rel[r], tg - P.cum[r], h, rem - h * S, S, H, C, slope,
                    lane);
  }
}

int gat_grid(int64_t waves_needed) {
  const int64_t w = std::min<int64_t>(waves_needed, (int64_t)kMaxBlocks * 4);
  return (int)std::min<int64_t>((w * kWave + kBlock - 1) / kBlock,
                                kMaxBlocks);
}

// fill the chip: split segments when (t, h) waves alone are few
int64_t gat_bwd_split(int64_t n_items) {
  const int64_t S = 32768 / std::max<int64_t>(n_items, 1);
  return std::max<int64_t>(1, std::min<int64_t>(S, 8));
}

template <typename Fn>
void gat_dispatch(bool bf16, Fn&& fn) {
  if (bf16) fn(__bf16{});
  else fn(float{});
}

// a size-1 dim may carry any stride
bool dense_inner(const torch::Tensor& x, int64_t C) {
  return (x.size(1) == 1 || x.stride(1) == C) &&
         (C == 1 || x.stride(2) == 1);
}

// Validates what forward and backward share and fills the pack with it: the
// inputs and each relation's slice of the (out, m, Z, s_pre) arenas.
// h views may be row-strided; dims 1, 2 must be dense.
template <typename T>
GatPack<T> gat_pack(const std::vector<torch::Tensor>& h_tgt,
                    const std::vector<torch::Tensor>& h_src,
                    const std::vector<torch::Tensor>& att_src,
                    const std::vector<torch::Tensor>& att_dst,
                    const std::vector<torch::Tensor>& src,
                    const std::vector<torch::Tensor>& off,
                    const torch::Tensor& out, const torch::Tensor& m,
                    const torch::Tensor& z, const torch::Tensor& spre) {
  const int R = (int)h_tgt.size();
  TORCH_CHECK(R >= 1 && R <= kMaxRel, "1..8 relations supported");
  const int64_t H = h_src[0].size(1), C = h_src[0].size(2);
  TORCH_CHECK(C <= 2 * kWave, "GAT fused kernel supports C <= 128");
  GatPack<T> P{};
  P.n_rel = R;
  int64_t e_off = 0;
  for (int r = 0; r < R; ++r) {
    const int64_t n_tgt = off[r].numel() - 1, nt_off = P.cum[r];
    TORCH_CHECK(dense_inner(h_tgt[r], C) && dense_inner(h_src[r], C),
                "gat: inner dims must be dense");
    TORCH_CHECK(h_tgt[r].size(0) >= n_tgt, "h_tgt must cover all targets");
    GatRel<T>& rel = P.rel[r];
    rel.h_tgt = reinterpret_cast<const T*>(h_tgt[r].data_ptr());
    rel.h_src = reinterpret_cast<const T*>(h_src[r].data_ptr());
    rel.tgt_stride = h_tgt[r].stride(0);
    rel.src_stride = h_src[r].stride(0);
    rel.att_src = att_src[r].data_ptr<float>();
    rel.att_dst = att_dst[r].data_ptr<float>();
    rel.src = src[r].data_ptr<int64_t>();
    rel.off = off[r].data_ptr<int64_t>();
    rel.out = reinterpret_cast<T*>(out.data_ptr()) + nt_off * H * C;
    rel.m = m.data_ptr<float>() + nt_off * H;
    rel.z = z.data_ptr<float>() + nt_off * H;
    rel.spre = spre.data_ptr<float>() + e_off * H;
    P.cum[r + 1] = nt_off + n_tgt;
    e_off += src[r].numel();
  }
  return P;
}

}  // namespace

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_multi_fwd(const std::vector<torch::Tensor>& h_tgt,
                  const std::vector<torch::Tensor>& h_src,
                  const std::vector<torch::Tensor>& att_src,
                  const std::vector<torch::Tensor>& att_dst,
                  const std::vector<torch::Tensor>& src,
                  const std::vector<torch::Tensor>& off, double slope,
                  const std::vector<torch::Tensor>& bias) {
  TORCH_CHECK(!h_src.empty(), "1..8 relations supported");
  const int64_t H = h_src[0].size(1), C = h_src[0].size(2);
  int64_t nt_tot = 0, e_tot = 0;
  for (size_t r = 0; r < off.size(); ++r) {
    nt_tot += off[r].numel() - 1;
    e_tot += src[r].numel();
  }
  auto fopt = h_src[0].options().dtype(torch::kFloat32);
  auto out = torch::empty({nt_tot, H, C}, h_src[0].options());
  auto m = torch::empty({nt_tot, H}, fopt);
  auto z = torch::empty({nt_tot, H}, fopt);
  auto spre = torch::empty({e_tot, H}, fopt);
  gat_dispatch(h_src[0].scalar_type() == torch::kBFloat16, [&](auto tag) {
    using T = decltype(tag);
    GatPack<T> P = gat_pack<T>(h_tgt, h_src, att_src, att_dst, src, off, out,
                               m, z, spre);
    for (int r = 0; r < P.n_rel; ++r)
      if (r < (int)bias.size() && bias[r].defined() && bias[r].numel() > 0)
        P.rel[r].bias = bias[r].data_ptr<float>();
    const GatRel<T>& one = P.rel[0];
    if (nt_tot == 0) return;
    if (P.n_rel == 1 && !one.bias && one.tgt_stride == H * C &&
        one.src_stride == H * C)
      hipLaunchKernelGGL(gat_fwd_one_kernel<T>, dim3(gat_grid(nt_tot * H)),
                         dim3(kBlock), 0, current_stream(), one.h_tgt,
                         one.h_src, one.att_src, one.att_dst, one.src,
                         one.off, nt_tot, H, C, (float)slope, one.out, one.m,
                         one.z, one.spre);
    else
      hipLaunchKernelGGL(gat_fwd_kernel<T>, dim3(gat_grid(nt_tot * H)),
                         dim3(kBlock), 0, current_stream(), P, H, C,
                         (float)slope, nt_tot);
  });
  return {out, m, z, spre};
}

void hip_gat_multi_bwd(const std::vector<torch::Tensor>& h_tgt,
                       const std::vector<torch::Tensor>& h_src,
                       const std::vector<torch::Tensor>& att_src,
                       const std::vector<torch::Tensor>& att_dst,
                       const std::vector<torch::Tensor>& src,
                       const std::vector<torch::Tensor>& off,
                       const torch::Tensor& out, const torch::Tensor& m,
                       const torch::Tensor& z, const torch::Tensor& spre,
                       const torch::Tensor& dout,
                       const std::vector<torch::Tensor>& dh_tgt,
                       const std::vector<torch::Tensor>& dh_src,
                       const std::vector<torch::Tensor>& datt_src,
                       const std::vector<torch::Tensor>& datt_dst,
                       double slope) {
  TORCH_CHECK(!h_src.empty(), "1..8 relations supported");
  const int64_t H = h_src[0].size(1), C = h_src[0].size(2);
  auto dc = dout.contiguous();
  gat_dispatch(h_src[0].scalar_type() == torch::kBFloat16, [&](auto tag) {
    using T = decltype(tag);
    GatPack<T> P = gat_pack<T>(h_tgt, h_src, att_src, att_dst, src, off, out,
                               m, z, spre);
    for (int r = 0; r < P.n_rel; ++r) {
      TORCH_CHECK(dh_tgt[r].stride(1) == C && dh_src[r].stride(1) == C,
                  "gat_multi_bwd: dh inner dims must be dense");
      GatRel<T>& rel = P.rel[r];
      rel.dout = reinterpret_cast<const T*>(dc.data_ptr()) + P.cum[r] * H * C;
      rel.dh_tgt = dh_tgt[r].data_ptr<float>();
      rel.dh_src = dh_src[r].data_ptr<float>();
      rel.dht_stride = dh_tgt[r].stride(0);
      rel.dhs_stride = dh_src[r].stride(0);
      rel.datt_src = datt_src[r].data_ptr<float>();
      rel.datt_dst = datt_dst[r].data_ptr<float>();
    }
    const int64_t nt_tot = P.cum[P.n_rel];
    if (nt_tot > 0) {
      const int64_t S = gat_bwd_split(nt_tot * H);
      hipLaunchKernelGGL(gat_bwd_kernel<T>, dim3(gat_grid(nt_tot * H * S)),
                         dim3(kBlock), 0, current_stream(), P, H, C,
                         (float)slope, S, nt_tot);
    }
  });
}

// A single GATConv is the one-relation table: contiguous rows (stride H*C),
// no bias.  Its forward takes gat_fwd_one_kernel, its backward the pack.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_fused_fwd(
    const torch::Tensor& h_tgt, const torch::Tensor& h_src,
    const torch::Tensor& att_src, const torch::Tensor& att_dst,
    const torch::Tensor& src, const torch::Tensor& offsets, double slope) {
  return hip_gat_multi_fwd({h_tgt}, {h_src},
                           {att_src.to(torch::kFloat32).contiguous()},
                           {att_dst.to(torch::kFloat32).contiguous()}, {src},
                           {offsets}, slope, {});
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_fused_bwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
                  const torch::Tensor& att_src,
                  const torch::Tensor& att_dst, const torch::Tensor& src,
                  const torch::Tensor& offsets, const torch::Tensor& out,
                  const torch::Tensor& m, const torch::Tensor& z,
                  const torch::Tensor& spre, const torch::Tensor& dout,
                  double slope) {
  // grad arenas are always fp32 (atomic accumulation); the python
  // wrapper casts dh back to the h dtype once
  auto fopt = h_src.options().dtype(torch::kFloat32);
  auto dh_tgt = torch::zeros(h_tgt.sizes(), fopt);
  auto dh_src = torch::zeros(h_src.sizes(), fopt);
  auto das = torch::zeros(att_src.sizes(), fopt);
  auto dad = torch::zeros(att_dst.sizes(), fopt);
  hip_gat_multi_bwd({h_tgt}, {h_src},
                    {att_src.to(torch::kFloat32).contiguous()},
                    {att_dst.to(torch::kFloat32).contiguous()}, {src},
                    {offsets}, out, m, z, spre, dout, {dh_tgt}, {dh_src},
                    {das}, {dad}, slope);
  return {dh_tgt, dh_src, das, dad};
}

}  // namespace glt

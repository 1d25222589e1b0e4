/* Grouped, K-segmented bf16 MFMA GEMM for relational layers (gfx950).
 *
 * A hetero layer is one GEMM per target node type whose reduction runs
 * across relations (the RGCN formulation):
 *
 *   Y_g[i, :] = act( sum over segments s of g with i < M_s of
 *                    ( x_s[i, :] @ W_s^T + b_s ) )
 *
 * The per-relation composition launches one cast, one GEMM and one add per
 * segment and rounds every partial to bf16.  Here one launch computes all
 * groups; a workgroup keeps its fp32 accumulators across the segments of
 * its group and rounds once.
 *
 *  1. relation_prep_kernel: all fp32 master weights to one bf16 arena, as
 *     W_s [N, K_s] and (for the input gradient) W_s^T [K_s, Np], Np = N
 *     rounded up to 8 with zero columns.  One launch instead of S casts
 *     and S transposes.
 *  2. relation_gemm_kernel: the grouped forward.  Descriptors travel by
 *     value in the kernel argument; a workgroup finds (group, row tile,
 *     column tile) through a cumulative tile table, the group index goes
 *     through readfirstlane so every descriptor field is a scalar load.
 *     The same kernel computes the input gradients, one single-segment
 *     group per segment: A = dY_g[:M_s], "W" = W_s^T from the arena.
 *  3. relation_mask_kernel: dY_g masked by Y_g <= 0 and padded to Np
 *     columns (16-byte rows for 2. and 4.), all groups in one launch.
 *  4. relation_wgrad_kernel + relation_fold_kernel: dW_s = dY_g[:M_s]^T @
 *     x_s and db_s = colsum(dY_g[:M_s]) for all segments, split-K into
 *     per-chunk fp32 planes (no output atomics), folded in ascending chunk
 *     order by one launch: bit-reproducible.
 *
 * Tile of 2.: 64 rows x 128 columns, 4 waves as 2 x 2, each wave 32 x 64 =
 * 2 x 4 fragments of 16x16x32_bf16 (A lane l holds A[i=l&15][k=(l>>4)*8+e],
 * C/D col=l&15, row=(l>>4)*4+reg).  Node types of a few hundred rows share
 * the table with types of a few hundred thousand: 128 columns give the
 * small types twice the workgroups of a 256-wide tile and 24 KB of LDS let
 * six workgroups share a CU, while an A row tile is still read only N/128
 * times, by neighbouring workgroups (the column tile runs fastest).
 * The staged LDS images, the prefetching K loops and the store epilogues
 * of 2. and 4. are those of the dense wide kernels (hip_mfma_tile.h).
 */
#include <algorithm>
#include <vector>

#include "hip_common.h"
#include "hip_mfma_tile.h"
#include "../include/hip_ops.h"

// No packed fp32 arithmetic in this file's device code (the build has one
// flag set for all files, so the target feature is switched off here).
// hip_mfma_tile.h opens a scope of this same pragma around its functions,
// so they and the kernels they are inlined into have one feature set.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(GLT_NO_PACKED_FP32, apply_to = function)
#endif

namespace glt {

namespace {

// Pack limits: descriptors are kernel arguments (4 KB budget).  The IGBH
// layer is 4 groups and 11 segments; its input gradient is 11 groups.
constexpr int kMaxSeg = 16;
constexpr int kMaxGrp = 16;

constexpr int RBM = 64, RBN = 128;             // forward tile

struct RlSeg {
  const __bf16* A;      // [M, K], row stride lda
  const __bf16* W;      // [N, K] contiguous
  const float* bias;    // [N] or null
  int64_t lda;
  int M, K;
};
struct RlGrp {
  __bf16* C;            // [M, N] contiguous
  int M, N;
  int seg0, seg1;       // segment range in RlPack::seg
  int n_blk;            // column tiles
  int cum;              // tiles of the groups before this one
};
struct RlPack {
  RlSeg seg[kMaxSeg];
  RlGrp grp[kMaxGrp];
  int n_grp;
  int relu;
};
static_assert(sizeof(RlPack) <= 2048, "kernel-argument budget");

__global__ __launch_bounds__(256)
void relation_gemm_kernel(const RlPack P) {
  // A image, then the W image; the epilogue reuses the front
  alignas(16) __shared__ unsigned char smem[(RBM + RBN) * RM_ROW_BYTES];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 1;                // 32-row wave tile
  const int wn = wave & 1;                 // 64-column wave tile
  const int fi = lane & 15;                // fragment col
  const int fg = lane >> 4;                // fragment row group

  // work decode: blockIdx is uniform, readfirstlane tells the compiler
  const int wg = (int)blockIdx.x;
  int gi = 0;
  while (gi + 1 < P.n_grp && wg >= P.grp[gi + 1].cum) ++gi;
  gi = __builtin_amdgcn_readfirstlane(gi);
  const RlGrp& G = P.grp[gi];
  const int local = wg - G.cum;
  const int N = G.N, Mg = G.M;
  const int block_col = (local % G.n_blk) * RBN;   // column tile fastest
  const int block_row = (local / G.n_blk) * RBM;

  f32x4 acc[2][4] = {};

  // Segment loop outermost: the accumulators live across it.  A row tile
  // wholly beyond the segment's rows takes nothing from it; the rows of a
  // partly covered tile beyond M_s are staged as zeros.
  for (int s = G.seg0; s < G.seg1; ++s) {
    const RlSeg& S = P.seg[s];
    if (block_row >= S.M) continue;
    rm_k_loop<RBM, RBN, 2, 4>(smem, S.A, S.lda, S.M, S.W, N, S.K, block_row,
                              block_col, acc);
  }

  // Biases in segment order, in fp32, on the rows their segment covers;
  // then ReLU, the one rounding and the line stores.
  for (int s = G.seg0; s < G.seg1; ++s) {
    const float* __restrict__ bias = P.seg[s].bias;
    if (bias == nullptr) continue;
    const int Ms = P.seg[s].M;
    float bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = block_col + wn * 64 + j * 16 + fi;
      bv[j] = col < N ? bias[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (block_row + wm * 32 + i * 16 + fg * 4 + r < Ms) {
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j][r] += bv[j];
        }
  }
  const float none[4] = {};
  rm_store_lines<2, 4, true>(smem, acc, none, false, P.relu != 0, G.C, Mg, N,
                             block_row + wm * 32, block_col + wn * 64);
}

// ---------------------------------------------------------------------------
// Weight preparation: W_s (fp32 or bf16) -> bf16 W_s [N, K] (fp32 sources
// only) and W_s^T [K, Np], 32x32 tiles through LDS so both sides are
// coalesced.  blockIdx.y is the segment.
// ---------------------------------------------------------------------------
struct RpSeg {
  const void* src;      // [N, K] contiguous
  __bf16* w;            // [N, K] or null
  __bf16* wt;           // [K, Np] or null
  int N, K, Np;
  int is_f32;
};
struct RpPack {
  RpSeg seg[kMaxSeg];
};

__global__ __launch_bounds__(256)
void relation_prep_kernel(const RpPack P) {
  __shared__ __bf16 tile[32][34];
  const RpSeg& S = P.seg[blockIdx.y];
  const int N = S.N, K = S.K, Np = S.Np;
  const int t_n = (Np + 31) / 32, t_k = (K + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int t = blockIdx.x; t < t_n * t_k; t += gridDim.x) {
    const int n0 = (t / t_k) * 32, k0 = (t % t_k) * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + ty + 8 * i, k = k0 + tx;
      __bf16 v = (__bf16)0.f;
      if (n < N && k < K) {
        const int64_t at = (int64_t)n * K + k;
        v = S.is_f32 ? (__bf16) reinterpret_cast<const float*>(S.src)[at]
                     : reinterpret_cast<const __bf16*>(S.src)[at];
        if (S.w != nullptr) S.w[at] = v;
      }
      tile[ty + 8 * i][tx] = v;
    }
    __syncthreads();
    if (S.wt != nullptr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + ty + 8 * i, n = n0 + tx;
        if (k < K && n < Np) S.wt[(int64_t)k * Np + n] = tile[tx][ty + 8 * i];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// dYm_g [M, Np] = dY_g masked by Y_g <= 0 (threshold_backward), the columns
// N .. Np zero.  blockIdx.y is the group.
// ---------------------------------------------------------------------------
struct RmGrp {
  const __bf16* dY;     // [M, N] contiguous
  const __bf16* Y;      // [M, N] contiguous or null (no mask)
  __bf16* out;          // [M, Np]
  int64_t M;
  int N, Np;
};
struct RmPack {
  RmGrp grp[kMaxGrp];
};

__global__ __launch_bounds__(256)
void relation_mask_kernel(const RmPack P) {
  const RmGrp& G = P.grp[blockIdx.y];
  const int64_t total = G.M * G.Np;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t m = e / G.Np;
    const int n = (int)(e - m * G.Np);
    __bf16 v = (__bf16)0.f;
    if (n < G.N) {
      v = G.dY[m * G.N + n];
      if (G.Y != nullptr && (float)G.Y[m * G.N + n] <= 0.f) v = (__bf16)0.f;
    }
    G.out[e] = v;
  }
}

// ---------------------------------------------------------------------------
// Grouped weight gradient.  Per segment: C[M, N] = A[Kb, M]^T @ B[Kb, N]
// with A = dYm_g (M = N_g output features, row stride lda >= M a multiple
// of 8, columns M .. lda zero), B = x_s (N = K_s), Kb = M_s batch rows.
// Work item = (segment, k chunk, m tile, n tile) through a cumulative
// table; 128 x 128 tiles, 8 waves as 2 x 4, each 64 x 32.  Both operands
// are K-major, so a 64-row K step is staged as loaded into a swizzled
// [k][128] image and ds_read_b64_tr_b16 builds the fragments; the next
// step is prefetched across the MFMAs.  The n tile 0 item of each (chunk,
// m tile) also sums db from the staged A tile.  Chunk partials go to
// planes [M * N + M] of the segment's arena slice.
// ---------------------------------------------------------------------------
struct RwSeg {
  const __bf16* A;
  const __bf16* B;
  float* P;             // z planes
  int64_t lda, ldb, plane;
  int Kb, M, N;
  int m_t, n_t;
  int cum;              // work items of the segments before this one
  int with_db;
};
struct RwPack {
  RwSeg seg[kMaxSeg];
  int n_seg;
  int k_per_z;          // reduction rows per chunk, a multiple of 64
};
static_assert(sizeof(RwPack) <= 2048, "kernel-argument budget");

__global__ __launch_bounds__(512)
void relation_wgrad_kernel(const RwPack P) {
  alignas(16) __shared__ unsigned char As[KM_TILE_BYTES];   // [k][m]
  alignas(16) __shared__ unsigned char Bs[KM_TILE_BYTES];   // [k][n]
  __shared__ float dbs[KM_BT][4];

  const int wg = (int)blockIdx.x;
  int si = 0;
  while (si + 1 < P.n_seg && wg >= P.seg[si + 1].cum) ++si;
  si = __builtin_amdgcn_readfirstlane(si);
  const RwSeg& S = P.seg[si];
  int local = wg - S.cum;
  const int nt = local % S.n_t;            // n tile fastest
  local /= S.n_t;
  const int mt = local % S.m_t;
  const int chunk = local / S.m_t;
  const int M = S.M, N = S.N;
  const int a_cols = (M + 7) & ~7;         // readable columns of A
  const int block_row = mt * KM_BT, block_col = nt * KM_BT;
  const int kz0 = chunk * P.k_per_z;
  const int kz1 = min(kz0 + P.k_per_z, S.Kb);
  const bool do_db = S.with_db != 0 && nt == 0;

  // both widths are multiples of 8: no chunk straddles an edge
  f32x4 acc[4][2] = {};
  float dsum = 0.f;
  km_k_loop(As, Bs, S.A, S.lda, a_cols, false, S.B, S.ldb, N, false,
            block_row, block_col, kz0, kz1, do_db, acc, dsum);
  float* const Cz = S.P + (int64_t)chunk * S.plane;
  km_store_plane(Cz, Cz + (int64_t)M * N, dbs, M, N, block_row, block_col,
                 acc, do_db, dsum);
}


// out[e] = sum over chunks c, ascending, of P[c * plane + e]: dW and db of
// one segment per blockIdx.y, zeros for a segment without chunks.
struct RfSeg {
  const float* P;
  float* out;
  int64_t plane;        // chunk stride
  int64_t len;          // cells to fold: M * N, + M with db
  int z;
};
struct RfPack {
  RfSeg seg[kMaxSeg];
};

__global__ __launch_bounds__(256)
void relation_fold_kernel(const RfPack P) {
  const RfSeg& S = P.seg[blockIdx.y];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < S.len;
       e += (int64_t)gridDim.x * 256) {
    float v = 0.f;
    for (int c = 0; c < S.z; ++c) v += S.P[(int64_t)c * S.plane + e];
    S.out[e] = v;
  }
}

// --- host side ---------------------------------------------------------------

bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

const __bf16* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const __bf16*>(t.data_ptr());
}

// A [M, K] bf16 operand the kernels can stage: rows dense, 16-byte aligned.
void check_operand(const torch::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2,
              "relation_linear: ", what, " must be a 2-D bf16 device tensor");
  TORCH_CHECK(t.size(1) % 8 == 0 && t.size(1) >= 8,
              "relation_linear: ", what, " needs columns % 8 == 0");
  TORCH_CHECK(t.size(0) < (int64_t)1 << 31,
              "relation_linear: ", what, " has too many rows");
  if (t.size(0) > 0)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 8 == 0) &&
                    t.stride(1) == 1 && aligned16(t.data_ptr()),
                "relation_linear: ", what,
                " needs dense, 16-byte aligned rows");
}

// Orders the segments by group (stable), fills the tile table and launches.
// grp[g] has C, M, N set; seg_group[s] is the group of segs[s].
void launch_relation_gemm(const std::vector<RlSeg>& segs,
                          const std::vector<int64_t>& seg_group,
                          std::vector<RlGrp> grp, bool relu) {
  TORCH_CHECK(segs.size() <= (size_t)kMaxSeg && grp.size() <= (size_t)kMaxGrp,
              "relation_linear: at most ", kMaxSeg, " segments and ",
              kMaxGrp, " groups per launch");
  RlPack P{};
  int n = 0;
  int64_t total = 0;
  for (size_t g = 0; g < grp.size(); ++g) {
    grp[g].seg0 = n;
    for (size_t s = 0; s < segs.size(); ++s)
      if (seg_group[s] == (int64_t)g) P.seg[n++] = segs[s];
    grp[g].seg1 = n;
    grp[g].n_blk = (grp[g].N + RBN - 1) / RBN;
    TORCH_CHECK(total < (int64_t)1 << 30, "relation_linear: too many tiles");
    grp[g].cum = (int)total;
    total += (int64_t)((grp[g].M + RBM - 1) / RBM) * grp[g].n_blk;
    P.grp[g] = grp[g];
  }
  TORCH_CHECK(total < (int64_t)1 << 31, "relation_linear: too many tiles");
  P.n_grp = (int)grp.size();
  P.relu = relu ? 1 : 0;
  if (total == 0) return;  // nothing to write, no zero-sized launch
  hipLaunchKernelGGL(relation_gemm_kernel, dim3((uint32_t)total), dim3(256),
                     0, current_stream(), P);
}

}  // namespace

int64_t relation_linear_max_segments() { return kMaxSeg; }
int64_t relation_linear_max_groups() { return kMaxGrp; }

std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>>
hip_relation_linear_prep(const std::vector<torch::Tensor>& weights,
                         bool need_t) {
  const size_t S = weights.size();
  TORCH_CHECK(S <= (size_t)kMaxSeg, "relation_linear: at most ", kMaxSeg,
              " segments per launch");
  std::vector<torch::Tensor> w16(S), wt(S);
  if (S == 0) return {w16, wt};
  // arena offsets in elements, every piece 16-byte aligned
  std::vector<int64_t> w_off(S, -1), t_off(S, -1);
  int64_t total = 0;
  int max_tiles = 0;
  bool any = false;
  for (size_t s = 0; s < S; ++s) {
    const auto& w = weights[s];
    TORCH_CHECK(w.is_cuda() && w.dim() == 2 && w.is_contiguous() &&
                    (w.scalar_type() == torch::kFloat32 ||
                     w.scalar_type() == torch::kBFloat16),
                "relation_linear: weights must be contiguous 2-D fp32 or "
                "bf16 device tensors");
    TORCH_CHECK(w.size(0) < (1 << 24) && w.size(1) < (1 << 24),
                "relation_linear: weight too large");
    const int64_t N = w.size(0), K = w.size(1), Np = (N + 7) / 8 * 8;
    const bool f32 = w.scalar_type() == torch::kFloat32;
    if (f32 || !aligned16(w.data_ptr())) {
      w_off[s] = total;
      total += (N * K + 7) / 8 * 8;
    }
    if (need_t) {
      t_off[s] = total;
      total += K * Np;
    }
    if (N * K > 0 && (w_off[s] >= 0 || need_t)) {
      any = true;
      max_tiles = std::max<int>(
          max_tiles, (int)(((Np + 31) / 32) * ((K + 31) / 32)));
    }
  }
  auto arena = torch::empty(
      {total}, weights[0].options().dtype(torch::kBFloat16));
  RpPack P{};
  __bf16* base = reinterpret_cast<__bf16*>(arena.data_ptr());
  for (size_t s = 0; s < S; ++s) {
    const auto& w = weights[s];
    const int64_t N = w.size(0), K = w.size(1), Np = (N + 7) / 8 * 8;
    RpSeg& R = P.seg[s];
    R.src = w.data_ptr();
    R.is_f32 = w.scalar_type() == torch::kFloat32;
    R.N = (int)N;
    R.K = (int)K;
    R.Np = (int)Np;
    if (w_off[s] >= 0) {
      R.w = base + w_off[s];
      w16[s] = arena.narrow(0, w_off[s], N * K).view({N, K});
    } else {
      w16[s] = w;  // bf16 already: used in place
    }
    if (need_t) {
      R.wt = base + t_off[s];
      wt[s] = arena.narrow(0, t_off[s], K * Np).view({K, Np});
    }
  }
  if (any)
    hipLaunchKernelGGL(relation_prep_kernel,
                       dim3((uint32_t)std::min(max_tiles, 1024), (uint32_t)S),
                       dim3(256), 0, current_stream(), P);
  return {w16, wt};
}

std::vector<torch::Tensor> hip_relation_linear_fwd(
    const std::vector<torch::Tensor>& xs,
    const std::vector<torch::Tensor>& w16,
    const std::vector<torch::Tensor>& biases,
    const std::vector<int64_t>& group, const std::vector<int64_t>& rows,
    bool relu) {
  const size_t S = xs.size(), G = rows.size();
  TORCH_CHECK(w16.size() == S && biases.size() == S && group.size() == S,
              "relation_linear: one weight, bias slot and group per segment");
  TORCH_CHECK(S <= (size_t)kMaxSeg && G <= (size_t)kMaxGrp,
              "relation_linear: at most ", kMaxSeg, " segments and ",
              kMaxGrp, " groups per launch");
  std::vector<int64_t> n_of(G, -1);
  std::vector<RlSeg> segs(S);
  for (size_t s = 0; s < S; ++s) {
    const auto& x = xs[s];
    const auto& w = w16[s];
    check_operand(x, "x");
    TORCH_CHECK(group[s] >= 0 && group[s] < (int64_t)G,
                "relation_linear: group index out of range");
    TORCH_CHECK(rows[group[s]] >= x.size(0),
                "relation_linear: rows[g] must cover every segment of g");
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
                    w.dim() == 2 && w.is_contiguous() &&
                    w.size(1) == x.size(1) && aligned16(w.data_ptr()),
                "relation_linear: weight must be contiguous aligned bf16 "
                "[N, K_s]");
    int64_t& N = n_of[group[s]];
    TORCH_CHECK(N < 0 || N == w.size(0),
                "relation_linear: N differs inside a group");
    N = w.size(0);
    RlSeg& R = segs[s];
    R.A = bf16_ptr(x);
    R.W = bf16_ptr(w);
    R.bias = nullptr;
    if (biases[s].numel() > 0) {
      const auto& b = biases[s];
      TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kFloat32 &&
                      b.dim() == 1 && b.size(0) == N && b.is_contiguous(),
                  "relation_linear: bias must be contiguous fp32 [N]");
      R.bias = b.data_ptr<float>();
    }
    R.lda = x.size(0) > 1 ? x.stride(0) : x.size(1);
    R.M = (int)x.size(0);
    R.K = (int)x.size(1);
  }
  std::vector<torch::Tensor> ys(G);
  std::vector<RlGrp> grp(G);
  for (size_t g = 0; g < G; ++g) {
    TORCH_CHECK(rows[g] >= 0 && rows[g] < (int64_t)1 << 31,
                "relation_linear: rows out of range");
    const int64_t N = std::max<int64_t>(n_of[g], 0);
    const auto opt = S > 0 ? xs[0].options()
                           : torch::TensorOptions().dtype(torch::kBFloat16)
                                 .device(torch::kCUDA);
    ys[g] = torch::empty({rows[g], N}, opt);
    grp[g] = RlGrp{reinterpret_cast<__bf16*>(ys[g].data_ptr()), (int)rows[g],
                   (int)N, 0, 0, 0, 0};
  }
  launch_relation_gemm(segs, group, grp, relu);
  return ys;
}

std::vector<torch::Tensor> hip_relation_linear_mask(
    const std::vector<torch::Tensor>& dys,
    const std::vector<torch::Tensor>& ys) {
  const size_t G = dys.size();
  TORCH_CHECK(G <= (size_t)kMaxGrp && (ys.empty() || ys.size() == G),
              "relation_linear: one Y per dY, at most ", kMaxGrp, " groups");
  std::vector<torch::Tensor> out(G);
  RmPack P{};
  int64_t most = 0;
  for (size_t g = 0; g < G; ++g) {
    const auto& dy = dys[g];
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16 &&
                    dy.dim() == 2 && dy.is_contiguous(),
                "relation_linear: dY must be contiguous 2-D bf16");
    const int64_t M = dy.size(0), N = dy.size(1), Np = (N + 7) / 8 * 8;
    RmGrp& R = P.grp[g];
    R.dY = bf16_ptr(dy);
    R.Y = nullptr;
    if (!ys.empty()) {
      TORCH_CHECK(ys[g].sizes() == dy.sizes() && ys[g].is_contiguous() &&
                      ys[g].scalar_type() == torch::kBFloat16,
                  "relation_linear: Y must match dY");
      R.Y = bf16_ptr(ys[g]);
    }
    if (R.Y == nullptr && Np == N && aligned16(dy.data_ptr())) {
      out[g] = dy;  // nothing to mask or pad
      R.M = 0;
      continue;
    }
    out[g] = torch::empty({M, Np}, dy.options());
    R.out = reinterpret_cast<__bf16*>(out[g].data_ptr());
    R.M = M;
    R.N = (int)N;
    R.Np = (int)Np;
    most = std::max(most, M * Np);
  }
  if (most > 0)
    hipLaunchKernelGGL(relation_mask_kernel,
                       dim3((uint32_t)grid_for(most), (uint32_t)G), dim3(256),
                       0, current_stream(), P);
  return out;
}

std::vector<torch::Tensor> hip_relation_linear_dgrad(
    const std::vector<torch::Tensor>& dym,
    const std::vector<torch::Tensor>& wt,
    const std::vector<int64_t>& group, const std::vector<int64_t>& seg_rows) {
  const size_t S = wt.size();
  TORCH_CHECK(group.size() == S && seg_rows.size() == S,
              "relation_linear: one group and row count per segment");
  std::vector<torch::Tensor> dxs(S);
  std::vector<RlSeg> segs(S);
  std::vector<RlGrp> grp(S);
  std::vector<int64_t> own(S);
  for (size_t s = 0; s < S; ++s) {
    TORCH_CHECK(group[s] >= 0 && group[s] < (int64_t)dym.size(),
                "relation_linear: group index out of range");
    const auto& dy = dym[group[s]];
    const auto& w = wt[s];
    check_operand(dy, "dY");
    check_operand(w, "W^T");
    TORCH_CHECK(w.is_contiguous() && w.size(1) == dy.size(1) &&
                    seg_rows[s] >= 0 && seg_rows[s] <= dy.size(0),
                "relation_linear: W^T [K_s, Np] must match dY [M, Np]");
    const int64_t Ms = seg_rows[s], Ks = w.size(0);
    dxs[s] = torch::empty({Ms, Ks}, dy.options());
    segs[s] = RlSeg{bf16_ptr(dy), bf16_ptr(w), nullptr,
                    dy.size(0) > 1 ? dy.stride(0) : dy.size(1), (int)Ms,
                    (int)dy.size(1)};
    grp[s] = RlGrp{reinterpret_cast<__bf16*>(dxs[s].data_ptr()), (int)Ms,
                   (int)Ks, 0, 0, 0, 0};
    own[s] = (int64_t)s;
  }
  launch_relation_gemm(segs, own, grp, false);
  return dxs;
}

std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>>
hip_relation_linear_wgrad(const std::vector<torch::Tensor>& dym,
                          const std::vector<torch::Tensor>& xs,
                          const std::vector<int64_t>& group,
                          const std::vector<int64_t>& n_out,
                          const std::vector<bool>& with_db) {
  const size_t S = xs.size();
  TORCH_CHECK(S <= (size_t)kMaxSeg, "relation_linear: at most ", kMaxSeg,
              " segments per launch");
  TORCH_CHECK(group.size() == S && n_out.size() == S && with_db.size() == S,
              "relation_linear: one group, N and db flag per segment");
  std::vector<torch::Tensor> dws(S), dbs(S);
  if (S == 0) return {dws, dbs};
  RwPack P{};
  RfPack F{};
  // chunks of equal length for every segment, sized so that the call has
  // about 1024 work items: known from the shapes, without a sync
  int64_t steps = 0;
  for (size_t s = 0; s < S; ++s) {
    TORCH_CHECK(group[s] >= 0 && group[s] < (int64_t)dym.size(),
                "relation_linear: group index out of range");
    const auto& dy = dym[group[s]];
    const auto& x = xs[s];
    check_operand(dy, "dY");
    check_operand(x, "x");
    const int64_t M = n_out[s], N = x.size(1), Kb = x.size(0);
    TORCH_CHECK(M >= 1 && (M + 7) / 8 * 8 == dy.size(1) && Kb <= dy.size(0),
                "relation_linear: dY [>= M_s, Np] must match x and N");
    RwSeg& R = P.seg[s];
    R.A = bf16_ptr(dy);
    R.B = bf16_ptr(x);
    R.lda = dy.size(0) > 1 ? dy.stride(0) : dy.size(1);
    R.ldb = Kb > 1 ? x.stride(0) : N;
    R.plane = M * N + M;
    R.Kb = (int)Kb;
    R.M = (int)M;
    R.N = (int)N;
    R.m_t = (int)((M + KM_BT - 1) / KM_BT);
    R.n_t = (int)((N + KM_BT - 1) / KM_BT);
    R.with_db = with_db[s] ? 1 : 0;
    steps += (int64_t)R.m_t * R.n_t * ((Kb + MT_BK - 1) / MT_BK);
  }
  const int64_t k_per_z = std::max<int64_t>(1, (steps + 1023) / 1024) * MT_BK;
  int64_t planes = 0, outs = 0, items = 0, most = 0;
  std::vector<int64_t> z(S), p_off(S), o_off(S);
  for (size_t s = 0; s < S; ++s) {
    RwSeg& R = P.seg[s];
    z[s] = (R.Kb + k_per_z - 1) / k_per_z;
    p_off[s] = planes;
    o_off[s] = outs;
    planes += z[s] * R.plane;
    outs += R.plane;
    R.cum = (int)items;
    items += z[s] * R.m_t * R.n_t;
    TORCH_CHECK(items < (int64_t)1 << 30, "relation_linear: too many tiles");
    most = std::max(most, R.plane);
  }
  const auto fopt = xs[0].options().dtype(torch::kFloat32);
  auto parts = torch::empty({std::max<int64_t>(planes, 1)}, fopt);
  auto out = torch::empty({outs}, fopt);
  for (size_t s = 0; s < S; ++s) {
    RwSeg& R = P.seg[s];
    R.P = parts.data_ptr<float>() + p_off[s];
    const int64_t M = R.M, N = R.N;
    // without with_db the db cells of the planes are never written
    F.seg[s] = RfSeg{R.P, out.data_ptr<float>() + o_off[s], R.plane,
                     with_db[s] ? R.plane : M * N, (int)z[s]};
    dws[s] = out.narrow(0, o_off[s], M * N).view({M, N});
    if (with_db[s]) dbs[s] = out.narrow(0, o_off[s] + M * N, M);
  }
  P.n_seg = (int)S;
  P.k_per_z = (int)k_per_z;
  if (items > 0)
    hipLaunchKernelGGL(relation_wgrad_kernel, dim3((uint32_t)items),
                       dim3(512), 0, current_stream(), P);
  hipLaunchKernelGGL(relation_fold_kernel,
                     dim3((uint32_t)grid_for(most), (uint32_t)S), dim3(256),
                     0, current_stream(), F);
  return {dws, dbs};
}

}  // namespace glt

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

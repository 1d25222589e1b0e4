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
 * Operands are K-innermost in memory and staged as loaded: 16-byte LDS
 * writes into an XOR-swizzled [row][64] image, the next K step prefetched
 * into registers across the MFMAs without a branch around the loads, zero
 * padding instead of masked lanes, and line-wide epilogue stores.
 */
#include <algorithm>
#include <vector>

#include "hip_common.h"
#include "../include/hip_ops.h"

// No packed fp32 arithmetic in this file's device code (the build has one
// flag set for all files, so the target feature is switched off here).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                            \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace glt {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4g;
typedef __attribute__((ext_vector_type(4))) short i16x4;

// Pack limits: descriptors are kernel arguments (4 KB budget).  The IGBH
// layer is 4 groups and 11 segments; its input gradient is 11 groups.
constexpr int kMaxSeg = 16;
constexpr int kMaxGrp = 16;

constexpr int RBM = 64, RBN = 128, RBK = 64;   // forward tile, K step
constexpr int R_ROW_BYTES = RBK * 2;           // one staged row: 64 k
constexpr int R_EP_LD = 68;                    // epilogue row stride, floats
constexpr int R_RPP = 32;                      // rows per staging pass

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

// Byte offset of 16-byte chunk `ch` (k = 8 ch .. 8 ch + 7) of row `row` in
// a staged image.  Rows are 128 bytes; XOR-ing the chunk with bits 1..3 of
// the row spreads the 8 lanes of a 16-byte store group (8 chunks of one
// row) and the 16 lanes of a fragment read group (16 rows at chunks c and
// c ^ 1) over all 64 banks.
__device__ __forceinline__ int rl_tile_off(int row, int ch) {
  return R_ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

// This thread's 16-byte chunks of the K step at k0: chunk s_ch of rows
// row0 + s_row + 32 h of X[rows, K] (row stride ld).  rl_issue starts the
// loads without a branch: a row past `rows` reads the last row and a chunk
// past K reads chunk 0 (in bounds: rows >= 1, K >= 8, K % 8 == 0).
// rl_finish, at LDS-write time, zeroes what was out of range.
template <int NV>
__device__ __forceinline__ void rl_issue(const __bf16* __restrict__ X,
                                         int rows, int K, int64_t ld,
                                         int row0, int k0, int s_row,
                                         int s_ch, bf16x8 (&v)[NV]) {
  const int k = k0 + s_ch * 8;
  const int kc = k + 8 <= K ? k : 0;
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    const int g_row = min(row0 + s_row + R_RPP * h, rows - 1);
    v[h] = *reinterpret_cast<const bf16x8*>(&X[(int64_t)g_row * ld + kc]);
  }
}

template <int NV>
__device__ __forceinline__ void rl_finish(int rows, int K, int row0, int k0,
                                          int s_row, int s_ch,
                                          bf16x8 (&v)[NV]) {
  const bool k_in = k0 + s_ch * 8 + 8 <= K;
#pragma unroll
  for (int h = 0; h < NV; ++h)
    if (!(k_in && row0 + s_row + R_RPP * h < rows)) v[h] = bf16x8{};
}

__global__ __launch_bounds__(256)
void relation_gemm_kernel(const RlPack P) {
  constexpr int NA = RBM / R_RPP, NB = RBN / R_RPP;
  // A image, then the W image; the epilogue reuses the front
  alignas(16) __shared__ unsigned char smem[(RBM + RBN) * R_ROW_BYTES];
  static_assert(4 * 16 * R_EP_LD * 4 <= (RBM + RBN) * R_ROW_BYTES,
                "epilogue tiles fit in the staging buffers");
  unsigned char* const As = smem;
  unsigned char* const Bs = smem + RBM * R_ROW_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1;                // 32-row wave tile
  const int wn = wave & 1;                 // 64-column wave tile

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
  // a wave whose 64 columns all lie past N multiplies nothing
  const bool live = block_col + wn * 64 < N;

  f32x4g acc[2][4] = {};

  const int s_row = tid >> 3;              // 8 lanes take one row's chunks
  const int s_ch = tid & 7;
  const int fi = lane & 15;                // fragment row / col
  const int fg = lane >> 4;                // fragment k group

  // Segment loop outermost: the accumulators live across it.
  for (int s = G.seg0; s < G.seg1; ++s) {
    const RlSeg& S = P.seg[s];
    const int Ms = S.M, K = S.K;
    // a row tile wholly beyond the segment's rows takes nothing from it
    if (block_row >= Ms || K <= 0) continue;
    const __bf16* __restrict__ A = S.A;
    const __bf16* __restrict__ W = S.W;
    const int64_t lda = S.lda;

    bf16x8 va[NA], vb[NB];
    rl_issue<NA>(A, Ms, K, lda, block_row, 0, s_row, s_ch, va);
    rl_issue<NB>(W, N, K, K, block_col, 0, s_row, s_ch, vb);

    for (int k0 = 0; k0 < K; k0 += RBK) {
      // rows of a partly covered tile beyond Ms are staged as zeros
      rl_finish<NA>(Ms, K, block_row, k0, s_row, s_ch, va);
      rl_finish<NB>(N, K, block_col, k0, s_row, s_ch, vb);
#pragma unroll
      for (int h = 0; h < NA; ++h)
        *reinterpret_cast<bf16x8*>(
            As + rl_tile_off(s_row + R_RPP * h, s_ch)) = va[h];
#pragma unroll
      for (int h = 0; h < NB; ++h)
        *reinterpret_cast<bf16x8*>(
            Bs + rl_tile_off(s_row + R_RPP * h, s_ch)) = vb[h];
      __syncthreads();
      if (k0 + RBK < K) {
        rl_issue<NA>(A, Ms, K, lda, block_row, k0 + RBK, s_row, s_ch, va);
        rl_issue<NB>(W, N, K, K, block_col, k0 + RBK, s_row, s_ch, vb);
      }
#pragma unroll
      for (int kk = 0; kk < RBK; kk += 32) {
        // a kk step past K holds only zero padding
        if (live && k0 + kk < K) {
          bf16x8 a[2], b[4];
#pragma unroll
          for (int i = 0; i < 2; ++i)
            a[i] = *reinterpret_cast<const bf16x8*>(
                As + rl_tile_off(wm * 32 + i * 16 + fi, (kk >> 3) + fg));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            b[j] = *reinterpret_cast<const bf16x8*>(
                Bs + rl_tile_off(wn * 64 + j * 16 + fi, (kk >> 3) + fg));
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[i], b[j], acc[i][j], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

  // Epilogue.  Biases in segment order, in fp32, on the rows their segment
  // covers; ReLU; then each wave passes its 32x64 tile, 16 rows at a time,
  // through its own [16][68] fp32 LDS tile and writes 128-byte row pieces,
  // 16 bytes per lane, rounded once here.  Rows of C start 16-byte aligned
  // only if N % 8 == 0; otherwise, and in the N tail, element stores.
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
  float* const ep = reinterpret_cast<float*>(smem) + wave * (16 * R_EP_LD);
  const bool relu = P.relu != 0;
  const bool vec_ok = N % 8 == 0;
  const int e_row = lane >> 3;
  const int e_col = (lane & 7) * 8;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r];
        if (relu) v = v > 0.f ? v : 0.f;
        ep[(fg * 4 + r) * R_EP_LD + j * 16 + fi] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rr = e_row + 8 * h;
      const int row = block_row + wm * 32 + i * 16 + rr;
      const int col = block_col + wn * 64 + e_col;
      const float* src = ep + rr * R_EP_LD + e_col;
      const f32x4g lo = *reinterpret_cast<const f32x4g*>(src);
      const f32x4g hi = *reinterpret_cast<const f32x4g*>(src + 4);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (__bf16)lo[e];
        o[4 + e] = (__bf16)hi[e];
      }
      if (row < Mg && col < N) {
        __bf16* dst = G.C + (int64_t)row * N + col;
        if (vec_ok && col + 7 < N) {
          *reinterpret_cast<bf16x8*>(dst) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (col + e < N) dst[e] = o[e];
        }
      }
    }
    __syncthreads();
  }
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
constexpr int WBT = 128;                       // tile edge
constexpr int W_ROW_BYTES = WBT * 2;

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

// Byte offset of 16-byte chunk `ch` (0..15) of k row `row` (0..63).  The
// XOR spreads the 8-lane groups of a 16-byte store and the two 4-row
// blocks a 32-lane half reads transposed over all banks.
__device__ __forceinline__ int rw_tile_off(int row, int ch) {
  return W_ROW_BYTES * row +
         16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// 16x16x32 operand fragment for columns 8 c0 .. 8 c0 + 15 (c0 even) and k
// rows r0 .. r0 + 7: lane (fi, g) ends with column fi, rows r0 + 0..7.
// Each transposed read takes a 4-row block; lane 4q + p of a 16-lane group
// addresses row q, elements 4p .. 4p + 3.  All lanes must be active.
__device__ __forceinline__ bf16x8 rw_frag(const unsigned char* tile, int r0,
                                          int c0, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3;
  typedef __attribute__((address_space(3))) i16x4* lds_i16x4;
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + rw_tile_off(r0 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + rw_tile_off(r0 + 4 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  return __builtin_bit_cast(
      bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// Rows k0 + s_row + {0, 32}, columns col0 .. col0 + 7 of X[., cols] (row
// stride ld; cols a multiple of 8, so a chunk is wholly in or out).  The
// loads start without a branch (a row past kz1 reads row kz1 - 1, a chunk
// past cols reads columns 0..7); rw_finish zeroes what was out of range.
__device__ __forceinline__ void rw_issue(const __bf16* __restrict__ X,
                                         int64_t ld, int cols, int col0,
                                         int k0, int kz1, int s_row,
                                         bf16x8 (&v)[2]) {
  const int c = col0 + 8 <= cols ? col0 : 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int g_k = min(k0 + s_row + 32 * h, kz1 - 1);
    v[h] = *reinterpret_cast<const bf16x8*>(&X[(int64_t)g_k * ld + c]);
  }
}

__device__ __forceinline__ void rw_finish(int cols, int col0, int k0,
                                          int kz1, int s_row,
                                          bf16x8 (&v)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (!(k0 + s_row + 32 * h < kz1 && col0 + 8 <= cols)) v[h] = bf16x8{};
}

__global__ __launch_bounds__(512)
void relation_wgrad_kernel(const RwPack P) {
  alignas(16) __shared__ unsigned char As[RBK * W_ROW_BYTES];   // [k][m]
  alignas(16) __shared__ unsigned char Bs[RBK * W_ROW_BYTES];   // [k][n]
  __shared__ float dbs[WBT][4];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 2;                // 64 rows each
  const int wn = wave & 3;                 // 32 cols each

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
  const int block_row = mt * WBT, block_col = nt * WBT;
  const int kz0 = chunk * P.k_per_z;
  const int kz1 = min(kz0 + P.k_per_z, S.Kb);
  const __bf16* __restrict__ A = S.A;
  const __bf16* __restrict__ B = S.B;

  f32x4g acc[4][2] = {};

  const int s_row = tid >> 4;              // 0..31 (+32)
  const int s_ch = tid & 15;
  const int fg8 = (lane >> 4) * 8;

  // db: thread (m_l, phase) sums rows phase, phase + 4, ... of column m_l
  const int m_l = tid & 127, phase = tid >> 7;
  const bool do_db = S.with_db != 0 && nt == 0;
  float dsum = 0.f;

  const int a_col = block_row + s_ch * 8, b_col = block_col + s_ch * 8;
  bf16x8 va[2], vb[2];
  rw_issue(A, S.lda, a_cols, a_col, kz0, kz1, s_row, va);
  rw_issue(B, S.ldb, N, b_col, kz0, kz1, s_row, vb);

  for (int k0 = kz0; k0 < kz1; k0 += RBK) {
    rw_finish(a_cols, a_col, k0, kz1, s_row, va);
    rw_finish(N, b_col, k0, kz1, s_row, vb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<bf16x8*>(
          As + rw_tile_off(s_row + 32 * h, s_ch)) = va[h];
      *reinterpret_cast<bf16x8*>(
          Bs + rw_tile_off(s_row + 32 * h, s_ch)) = vb[h];
    }
    __syncthreads();
    if (k0 + RBK < kz1) {
      rw_issue(A, S.lda, a_cols, a_col, k0 + RBK, kz1, s_row, va);
      rw_issue(B, S.ldb, N, b_col, k0 + RBK, kz1, s_row, vb);
    }
#pragma unroll
    for (int kk = 0; kk < RBK; kk += 32) {
      bf16x8 a[4], b[2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = rw_frag(As, kk + fg8, wm * 8 + i * 2, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = rw_frag(Bs, kk + fg8, wn * 4 + j * 2, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (do_db) {
      // ascending k; the zero rows past kz1 add +0
#pragma unroll
      for (int r = 0; r < RBK; r += 4)
        dsum += (float)*reinterpret_cast<const __bf16*>(
            As + rw_tile_off(r + phase, m_l >> 3) + 2 * (m_l & 7));
    }
    __syncthreads();
  }

  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
  float* const Cz = S.P + (int64_t)chunk * S.plane;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = block_row + wm * 64 + i * 16 + c_row0 + r;
        const int col = block_col + wn * 32 + j * 16 + c_col;
        if (row < M && col < N) Cz[(int64_t)row * N + col] = acc[i][j][r];
      }
    }
  }
  if (do_db) {
    dbs[m_l][phase] = dsum;
    __syncthreads();
    if (tid < WBT && block_row + tid < M)
      Cz[(int64_t)M * N + block_row + tid] =
          dbs[tid][0] + dbs[tid][1] + dbs[tid][2] + dbs[tid][3];
  }
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
    R.m_t = (int)((M + WBT - 1) / WBT);
    R.n_t = (int)((N + WBT - 1) / WBT);
    R.with_db = with_db[s] ? 1 : 0;
    steps += (int64_t)R.m_t * R.n_t * ((Kb + RBK - 1) / RBK);
  }
  const int64_t k_per_z = std::max<int64_t>(1, (steps + 1023) / 1024) * RBK;
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

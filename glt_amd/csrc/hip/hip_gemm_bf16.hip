/* Hand-written bf16 MFMA GEMM family for GNN projection shapes (gfx950).
 *
 * Why: hipBLASLt's heuristic picks ~50 TF/s tiles for the tall-skinny
 * batches this framework produces (M~1e5, N=256, K=200/512 — measured
 * 322 us for the 17 GFLOP flagship projection, profiles/r02_*), a tiny
 * fraction of the 16x16x32_bf16 MFMA rate.  Three kernels:
 *
 *  1. gemm_bt_kernel:  C[M,N] = relu(A[M,K] @ Bt[N,K]^T + bias)
 *     - Bt is the nn.Linear weight layout [out,in] as-is: NO transpose
 *       materialization anywhere on the forward path.
 *     - bf16 in, bf16 out, fp32 accumulate, bias+ReLU fused in the
 *       epilogue (kills the separate activation round-trip).
 *     - two forms with bit-identical results, chosen by
 *       gemm_bt_bf16_plan: gemm_bt_wide_kernel (64 x 256 tiles: A read
 *       once, next K step prefetched across the MFMAs, swizzled 16-byte
 *       LDS traffic, whole-line stores) for the large projections, and
 *       the 64x64 gemm_bt_kernel for everything it cannot take (K not a
 *       multiple of 8, N < 128) or M too small to fill the CUs.
 *  2. gemm_kt_kernel:  dW[M,N] = A[Kb,M]^T @ B[Kb,N], db[M] = colsum(A)
 *     - the weight-gradient shape (K huge = batch rows): split-K over
 *       grid.z into per-chunk partial planes (a torch sum folds them);
 *       the bias gradient rides the same kernel (the separate
 *       [rows,256] bf16 column-reduce measured 78 us/call).
 *     - fp32 out: master-grad dtype, so the .to(fp32) casts disappear.
 *  3. mfma_bf16_selftest: one 16x16x32 / 32x32x16 tile from explicit
 *     matrices (fragment-layout ground truth for the GPU tests).
 *
 * Fragment layouts (cdna4 §10): 16x16x32_bf16: A lane l holds
 * A[i=l&15][k=(l>>4)*8+e], B lane l holds B[k=(l>>4)*8+e][j=l&15],
 * C/D col=l&15, row=(l>>4)*4+reg.  gemm_bt reads fragments as
 * contiguous 16-byte LDS vectors: A and Bt are staged row-major (their
 * K dim is innermost in global memory already).  The kt operands are
 * K-major in memory instead.  The 64x64 gemm_kt_kernel transposes them
 * during its LDS write pass (b32 writes of paired k rows) and reads the
 * same 16-byte vectors.  The 128x128 gemm_kt128_kernel does not
 * transpose: it stores each 16-byte global load as one 16-byte LDS write
 * into a swizzled [k][128] image and builds the fragments with the
 * transposed LDS read ds_read_b64_tr_b16 (two per operand), prefetches
 * the next K step into registers across the MFMAs, and sums db from the
 * staged A tile.  Lane (fi, g) still holds k = kk + 8g + 0..7 and the
 * MFMA order is unchanged, so dW and db are bit-for-bit those of the
 * transposing kernel it replaces.
 */
#include <cstdlib>
#include <string>

#include "hip_common.h"
#include "../include/common.h"
#include "../include/hip_ops.h"

namespace glt {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4b;

constexpr int GBM = 64, GBN = 64, GBK = 64;  // block tile
constexpr int LDP = 8;                       // LDS row pad (bf16 elems)

__device__ __forceinline__ float bf2f(__bf16 v) { return (float)v; }
__device__ __forceinline__ __bf16 f2bf(float v) { return (__bf16)v; }

// C[M,N] = act(A[M,K] @ Bt[N,K]^T + bias).  4 waves as 2x2; each wave a
// 32x32 tile of 2x2 16x16 fragments; K staged in GBK=64 steps.
template <bool RELU, bool BF16_OUT>
__global__ __launch_bounds__(256)
void gemm_bt_kernel(const __bf16* __restrict__ A,
                    const __bf16* __restrict__ Bt,
                    const float* __restrict__ bias,
                    void* __restrict__ Cv,
                    int64_t M, int64_t K, int64_t N) {
  __shared__ __bf16 As[GBM][GBK + LDP];
  __shared__ __bf16 Bs[GBN][GBK + LDP];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;            // 32-row wave tile
  const int wc = wave & 1;             // 32-col wave tile

  const int64_t block_row = (int64_t)blockIdx.x * GBM;
  const int64_t block_col = (int64_t)blockIdx.y * GBN;

  f32x4b acc[2][2] = {};

  // staging map: 256 threads, each loads 16 bf16 (32 B) per row set;
  // a 64x64 bf16 tile is 256 x 16 elements.
  const int s_row = tid >> 2;          // 0..63
  const int s_col = (tid & 3) * 16;    // 0,16,32,48

  const int fi = lane & 15;            // fragment row/col
  const int fk8 = (lane >> 4) * 8;     // fragment k base

  for (int64_t k0 = 0; k0 < K; k0 += GBK) {
    const int64_t kmax = K - k0;
    // stage A row-major
    {
      const int64_t g_row = block_row + s_row;
      bf16x8 v0 = {}, v1 = {};
      if (g_row < M) {
        const int64_t base = g_row * K + k0 + s_col;
        if (s_col + 15 < kmax) {
          v0 = *reinterpret_cast<const bf16x8*>(&A[base]);
          v1 = *reinterpret_cast<const bf16x8*>(&A[base + 8]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (s_col + e < kmax) v0[e] = A[base + e];
            if (s_col + 8 + e < kmax) v1[e] = A[base + 8 + e];
          }
        }
      }
      *reinterpret_cast<bf16x8*>(&As[s_row][s_col]) = v0;
      *reinterpret_cast<bf16x8*>(&As[s_row][s_col + 8]) = v1;
    }
    // stage Bt row-major (same geometry: rows are output cols)
    {
      const int64_t g_row = block_col + s_row;
      bf16x8 v0 = {}, v1 = {};
      if (g_row < N) {
        const int64_t base = g_row * K + k0 + s_col;
        if (s_col + 15 < kmax) {
          v0 = *reinterpret_cast<const bf16x8*>(&Bt[base]);
          v1 = *reinterpret_cast<const bf16x8*>(&Bt[base + 8]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (s_col + e < kmax) v0[e] = Bt[base + e];
            if (s_col + 8 + e < kmax) v1[e] = Bt[base + 8 + e];
          }
        }
      }
      *reinterpret_cast<bf16x8*>(&Bs[s_row][s_col]) = v0;
      *reinterpret_cast<bf16x8*>(&Bs[s_row][s_col + 8]) = v1;
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < GBK; kk += 32) {
      // NOTE: mfma B fragment is B[k][j]; our Bs rows are j with k
      // contiguous — exactly the A-layout, and A@Bt^T is symmetric in
      // (A,Bt), so both fragments load the same way.
      bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + fi][kk + fk8]);
      bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + 16 + fi][kk + fk8]);
      bf16x8 b0 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + fi][kk + fk8]);
      bf16x8 b1 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + 16 + fi][kk + fk8]);
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0,
                                                          acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1,
                                                          acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0,
                                                          acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1,
                                                          acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // C/D: col = lane&15, row = (lane>>4)*4 + reg.
  // mfma computed acc = As_frag @ Bs_frag^T with both fragments in
  // "A layout": result row i = A row, result col j = Bs row = output col.
  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
#pragma unroll
  for (int fi2 = 0; fi2 < 2; ++fi2) {
#pragma unroll
    for (int fj = 0; fj < 2; ++fj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = block_row + wr * 32 + fi2 * 16 + c_row0 + r;
        const int64_t col = block_col + wc * 32 + fj * 16 + c_col;
        if (row < M && col < N) {
          float v = acc[fi2][fj][r];
          if (bias != nullptr) v += bias[col];
          if (RELU) v = v > 0.f ? v : 0.f;
          if (BF16_OUT)
            reinterpret_cast<__bf16*>(Cv)[row * N + col] = f2bf(v);
          else
            reinterpret_cast<float*>(Cv)[row * N + col] = v;
        }
      }
    }
  }
}


// Persistent-B forward variant for K <= 256: the whole Bt n-tile
// ([64][K] bf16 <= 32 KB) is staged ONCE per workgroup, then A m-tiles
// stream through with a single sync pair each and one full-K MFMA pass
// — the generic kernel re-stages B and syncs per 64-K step.
constexpr int PKP = 256;  // padded K capacity

template <bool RELU, bool BF16_OUT>
__global__ __launch_bounds__(256)
void gemm_bt_persist_kernel(const __bf16* __restrict__ A,
                            const __bf16* __restrict__ Bt,
                            const float* __restrict__ bias,
                            void* __restrict__ Cv,
                            int64_t M, int64_t K, int64_t N) {
  __shared__ __bf16 As[GBM][PKP + LDP];
  __shared__ __bf16 Bs[GBN][PKP + LDP];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;
  const int64_t block_col = (int64_t)blockIdx.y * GBN;
  const int s_row = tid >> 2;          // 0..63
  const int s_col0 = (tid & 3) * 64;   // 4 threads cover 256 cols
  const int fi = lane & 15;
  const int fk8 = (lane >> 4) * 8;
  const int kp = (int)((K + 31) / 32) * 32;

  // stage Bt rows once (zero-padded K tail)
  {
    const int64_t g_row = block_col + s_row;
#pragma unroll
    for (int c8 = 0; c8 < 64; c8 += 8) {
      const int col = s_col0 + c8;
      bf16x8 v = {};
      if (col < kp && g_row < N) {
        const int64_t base = g_row * K + col;
        if (col + 7 < K) {
          v = *reinterpret_cast<const bf16x8*>(&Bt[base]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (col + e < K) v[e] = Bt[base + e];
        }
      }
      if (col < kp)
        *reinterpret_cast<bf16x8*>(&Bs[s_row][col]) = v;
    }
  }
  __syncthreads();

  for (int64_t m0 = (int64_t)blockIdx.x * GBM; m0 < M;
       m0 += (int64_t)gridDim.x * GBM) {
    {
      const int64_t g_row = m0 + s_row;
#pragma unroll
      for (int c8 = 0; c8 < 64; c8 += 8) {
        const int col = s_col0 + c8;
        bf16x8 v = {};
        if (col < kp && g_row < M) {
          const int64_t base = g_row * K + col;
          if (col + 7 < K) {
            v = *reinterpret_cast<const bf16x8*>(&A[base]);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (col + e < K) v[e] = A[base + e];
          }
        }
        if (col < kp)
          *reinterpret_cast<bf16x8*>(&As[s_row][col]) = v;
      }
    }
    __syncthreads();
    f32x4b acc[2][2] = {};
    for (int kk = 0; kk < kp; kk += 32) {
      bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + fi][kk + fk8]);
      bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + 16 + fi][kk + fk8]);
      bf16x8 b0 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + fi][kk + fk8]);
      bf16x8 b1 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + 16 + fi][kk + fk8]);
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0,
                                                          acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1,
                                                          acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0,
                                                          acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1,
                                                          acc[1][1], 0, 0, 0);
    }
    __syncthreads();
    const int c_col = lane & 15;
    const int c_row0 = (lane >> 4) * 4;
#pragma unroll
    for (int fi2 = 0; fi2 < 2; ++fi2) {
#pragma unroll
      for (int fj = 0; fj < 2; ++fj) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = m0 + wr * 32 + fi2 * 16 + c_row0 + r;
          const int64_t col = block_col + wc * 32 + fj * 16 + c_col;
          if (row < M && col < N) {
            float v = acc[fi2][fj][r];
            if (bias != nullptr) v += bias[col];
            if (RELU) v = v > 0.f ? v : 0.f;
            if (BF16_OUT)
              reinterpret_cast<__bf16*>(Cv)[row * N + col] = f2bf(v);
            else
              reinterpret_cast<float*>(Cv)[row * N + col] = v;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Wide forward tile: BM rows x 256 columns per workgroup, BM / 16 waves as
// (BM / 64) x 4, each wave a 64x64 tile of 4x4 16x16 fragments.  At
// N <= 256 every A row is fetched by exactly one workgroup; for N > 256
// the column block is the fast index of the 1-D grid, so the workgroups
// that share an A row tile are neighbours and the second read hits in L2.
//
// A and Bt are K-innermost in memory, so a 64-wide K step of either is
// staged as it is loaded: 16-byte LDS writes of the 16-byte global loads
// into a [row][64] image with 128-byte rows, XOR-swizzled (bt_tile_off),
// and 16-byte fragment reads.  The loads of step i+1 are issued into
// registers right after the barrier of step i and written to LDS after
// its MFMAs.  The MFMA, the lane-to-k map (lane group g holds
// k = kk + 8g .. +7) and the ascending kk order are those of
// gemm_bt_kernel, and a kk step of nothing but zero padding that is
// skipped here adds +0 there: outputs are bit-for-bit the same.
// ---------------------------------------------------------------------------
constexpr int WBN = 256;                   // output columns per workgroup
constexpr int BT_ROW_BYTES = GBK * 2;      // one staged row: 64 k
constexpr int BT_EP_LD = 68;               // epilogue row stride in floats

// Byte offset of 16-byte chunk `ch` (0..7: k = 8 ch .. 8 ch + 7) of row
// `row` in a staged image.  Rows are 128 bytes, so two rows fill the 64
// banks once; XOR-ing the chunk with bits 1..3 of the row makes the eight
// rows of one parity in any aligned 16-row block start in eight different
// 16-byte slots.  The 8 lanes of a 16-byte store group write the 8 chunks
// of one row (a permutation of the 8 slots), and the 16 lanes of a
// 16-byte read group, 8 rows at chunk c and 8 at chunk c ^ 1 of one
// aligned 16-row block, cover all 64 banks exactly once.
__host__ __device__ constexpr int bt_tile_off(int row, int ch) {
  return BT_ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

// This thread's 16-byte chunks of the K step at k0: chunk s_ch of rows
// row0 + s_row + RPP * h of X[rows, K].  bt_issue only starts the loads,
// without a branch: a row past `rows` reads the last row and a chunk past
// K reads chunk 0 (both in bounds: rows >= 1, K >= 32 and K % 8 == 0 on
// this path, so a chunk is wholly inside K or wholly outside).  bt_finish,
// at LDS-write time, zeroes what was out of range: the image is
// zero-padded, never masked.
template <int NV, int RPP>
__device__ __forceinline__ void bt_issue(const __bf16* __restrict__ X,
                                         int64_t rows, int64_t K,
                                         int64_t row0, int64_t k0, int s_row,
                                         int s_ch, bf16x8 (&v)[NV]) {
  const int64_t k = k0 + s_ch * 8;
  const int64_t kc = k + 8 <= K ? k : 0;
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    const int64_t g_row = std::min<int64_t>(row0 + s_row + RPP * h, rows - 1);
    v[h] = *reinterpret_cast<const bf16x8*>(&X[g_row * K + kc]);
  }
}

template <int NV, int RPP>
__device__ __forceinline__ void bt_finish(int64_t rows, int64_t K,
                                          int64_t row0, int64_t k0, int s_row,
                                          int s_ch, bf16x8 (&v)[NV]) {
  const bool k_in = k0 + s_ch * 8 + 8 <= K;
#pragma unroll
  for (int h = 0; h < NV; ++h)
    if (!(k_in && row0 + s_row + RPP * h < rows)) v[h] = bf16x8{};
}

template <int BM, bool RELU, bool BF16_OUT>
__global__ __launch_bounds__(BM * 4)
void gemm_bt_wide_kernel(const __bf16* __restrict__ A,
                         const __bf16* __restrict__ Bt,
                         const float* __restrict__ bias,
                         void* __restrict__ Cv,
                         int64_t M, int64_t K, int64_t N, int n_blk) {
  constexpr int NT = BM * 4;               // threads
  constexpr int RPP = NT / 8;              // rows one staging pass covers
  constexpr int NA = BM / RPP, NB = WBN / RPP;
  static_assert(BM % 64 == 0 && NA >= 1, "whole 64-row wave tiles");
  // A image, then the Bt image; the epilogue reuses the front of it
  alignas(16) __shared__ unsigned char smem[(BM + WBN) * BT_ROW_BYTES];
  static_assert((NT / 64) * 16 * BT_EP_LD * 4 <= (BM + WBN) * BT_ROW_BYTES,
                "epilogue tiles fit in the staging buffers");
  unsigned char* const As = smem;
  unsigned char* const Bs = smem + BM * BT_ROW_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 2;                // 64-row wave tile
  const int wn = wave & 3;                 // 64-col wave tile

  const int64_t block_col = (int64_t)(blockIdx.x % n_blk) * WBN;
  const int64_t block_row = (int64_t)(blockIdx.x / n_blk) * BM;
  // a wave whose 64 columns all lie past N multiplies nothing
  const bool live = block_col + wn * 64 < N;

  f32x4b acc[4][4] = {};

  // staging: 8 lanes take the 8 chunks of one row
  const int s_row = tid >> 3;
  const int s_ch = tid & 7;
  const int fi = lane & 15;                // fragment row / col
  const int fg = lane >> 4;                // fragment k group

  bf16x8 va[NA], vb[NB];
  if (K > 0) {
    bt_issue<NA, RPP>(A, M, K, block_row, 0, s_row, s_ch, va);
    bt_issue<NB, RPP>(Bt, N, K, block_col, 0, s_row, s_ch, vb);
  }

  for (int64_t k0 = 0; k0 < K; k0 += GBK) {
    bt_finish<NA, RPP>(M, K, block_row, k0, s_row, s_ch, va);
    bt_finish<NB, RPP>(N, K, block_col, k0, s_row, s_ch, vb);
#pragma unroll
    for (int h = 0; h < NA; ++h)
      *reinterpret_cast<bf16x8*>(
          As + bt_tile_off(s_row + RPP * h, s_ch)) = va[h];
#pragma unroll
    for (int h = 0; h < NB; ++h)
      *reinterpret_cast<bf16x8*>(
          Bs + bt_tile_off(s_row + RPP * h, s_ch)) = vb[h];
    __syncthreads();
    if (k0 + GBK < K) {
      bt_issue<NA, RPP>(A, M, K, block_row, k0 + GBK, s_row, s_ch, va);
      bt_issue<NB, RPP>(Bt, N, K, block_col, k0 + GBK, s_row, s_ch, vb);
    }

#pragma unroll
    for (int kk = 0; kk < GBK; kk += 32) {
      // a kk step past K holds only zero padding
      if (live && k0 + kk < K) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a[i] = *reinterpret_cast<const bf16x8*>(
              As + bt_tile_off(wm * 64 + i * 16 + fi, (kk >> 3) + fg));
#pragma unroll
        for (int j = 0; j < 4; ++j)
          b[j] = *reinterpret_cast<const bf16x8*>(
              Bs + bt_tile_off(wn * 64 + j * 16 + fi, (kk >> 3) + fg));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // Epilogue.  C/D: col = lane & 15, row = (lane >> 4) * 4 + reg.  Bias
  // and ReLU in fp32 as in gemm_bt_kernel, then each wave passes its
  // 64x64 tile, 16 rows at a time, through its own [16][68] fp32 LDS tile
  // (the staging buffers: every wave is past the last barrier above) and
  // writes whole row pieces, 16 bytes per lane: 8 lanes a 128-byte row
  // piece of bf16 (rounded once, here), 16 lanes 256 bytes of fp32.  The
  // 68-float stride puts the two rows a 32-lane half writes 16 banks
  // apart.  A row of C starts 16-byte aligned only if N is a multiple of
  // 8 (bf16) or 4 (fp32); otherwise, and in the N tail, elements are
  // stored one by one.
  float* const ep = reinterpret_cast<float*>(smem) + wave * (16 * BT_EP_LD);
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t col = block_col + wn * 64 + j * 16 + fi;
      if (col < N) bv[j] = bias[col];
    }
  }
  constexpr int CPL = BF16_OUT ? 8 : 4;    // columns per lane
  constexpr int LPR = 64 / CPL;            // lanes per 64-column row piece
  constexpr int RPI = 64 / LPR;            // rows per wave instruction
  const bool vec_ok = N % CPL == 0;
  const int e_row = lane / LPR;
  const int e_col = (lane % LPR) * CPL;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r];
        if (bias != nullptr) v += bv[j];
        if (RELU) v = v > 0.f ? v : 0.f;
        ep[(fg * 4 + r) * BT_EP_LD + j * 16 + fi] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 16 / RPI; ++h) {
      const int rr = e_row + RPI * h;
      const int64_t row = block_row + wm * 64 + i * 16 + rr;
      const int64_t col = block_col + wn * 64 + e_col;
      const float* src = ep + rr * BT_EP_LD + e_col;
      const f32x4b lo = *reinterpret_cast<const f32x4b*>(src);
      if (BF16_OUT) {
        const f32x4b hi = *reinterpret_cast<const f32x4b*>(src + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = f2bf(lo[e]);
          o[4 + e] = f2bf(hi[e]);
        }
        __bf16* dst = reinterpret_cast<__bf16*>(Cv) + row * N + col;
        if (row < M) {
          if (vec_ok && col + 7 < N) {
            *reinterpret_cast<bf16x8*>(dst) = o;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (col + e < N) dst[e] = o[e];
          }
        }
      } else {
        float* dst = reinterpret_cast<float*>(Cv) + row * N + col;
        if (row < M) {
          if (vec_ok && col + 3 < N) {
            *reinterpret_cast<f32x4b*>(dst) = lo;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < N) dst[e] = lo[e];
          }
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// dW[M,N] = A[Kb,M]^T @ B[Kb,N] (+ db[M] = colsum A), split-K over
// grid.z with per-chunk partial planes.  A/B tiles are transposed
// during the LDS write pass (paired k-rows -> b32 writes) so fragments
// read as contiguous 16-byte vectors for the bf16 16x16x32 MFMA.
// (An f32-16x16x4 variant with transpose-free fragments measured
// SLOWER — 40 vs 56 TF/s — the f32 MFMA issue rate is the wall.)
// ---------------------------------------------------------------------------
template <bool WITH_DB>
__global__ __launch_bounds__(256)
void gemm_kt_kernel(const __bf16* __restrict__ A,
                    const __bf16* __restrict__ B,
                    float* __restrict__ C,
                    float* __restrict__ db,
                    int64_t Kb, int64_t M, int64_t N, int64_t k_per_z,
                    int64_t plane) {
  __shared__ __bf16 As[GBM][GBK + LDP];   // As[m][k]
  __shared__ __bf16 Bs[GBN][GBK + LDP];   // Bs[n][k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;

  const int64_t block_row = (int64_t)blockIdx.x * GBM;   // m tile
  const int64_t block_col = (int64_t)blockIdx.y * GBN;   // n tile
  const int64_t kz0 = (int64_t)blockIdx.z * k_per_z;
  const int64_t kz1 = std::min(kz0 + k_per_z, Kb);

  f32x4b acc[2][2] = {};

  // transposing stage: thread owns TWO adjacent k rows x 8 cols, so
  // each LDS write is a b32 pair (halves the transpose instruction
  // count vs scalar b16 writes).  32 k-pairs x 8 col-groups = 256.
  const int t_k = (tid >> 3) * 2;      // 0..62 step 2
  const int t_c = (tid & 7) * 8;       // 0..56 step 8

  const int fi = lane & 15;
  const int fk8 = (lane >> 4) * 8;

  for (int64_t k0 = kz0; k0 < kz1; k0 += GBK) {
    const int64_t g_k = k0 + t_k;
    // stage A^T: As[m][k] = A[k][m]
    {
      bf16x8 v0 = {}, v1 = {};
      if (g_k < kz1 && block_row + t_c < M) {
        const int64_t base = g_k * M + block_row + t_c;
        if (block_row + t_c + 7 < M) {
          v0 = *reinterpret_cast<const bf16x8*>(&A[base]);
          if (g_k + 1 < kz1)
            v1 = *reinterpret_cast<const bf16x8*>(&A[base + M]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (block_row + t_c + e < M) {
              v0[e] = A[base + e];
              if (g_k + 1 < kz1) v1[e] = A[base + M + e];
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 pair[2] = {v0[e], v1[e]};
        *reinterpret_cast<uint32_t*>(&As[t_c + e][t_k]) =
            *reinterpret_cast<const uint32_t*>(pair);
      }
    }
    // stage B^T: Bs[n][k] = B[k][n]
    {
      bf16x8 v0 = {}, v1 = {};
      if (g_k < kz1 && block_col + t_c < N) {
        const int64_t base = g_k * N + block_col + t_c;
        if (block_col + t_c + 7 < N) {
          v0 = *reinterpret_cast<const bf16x8*>(&B[base]);
          if (g_k + 1 < kz1)
            v1 = *reinterpret_cast<const bf16x8*>(&B[base + N]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (block_col + t_c + e < N) {
              v0[e] = B[base + e];
              if (g_k + 1 < kz1) v1[e] = B[base + N + e];
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        __bf16 pair[2] = {v0[e], v1[e]};
        *reinterpret_cast<uint32_t*>(&Bs[t_c + e][t_k]) =
            *reinterpret_cast<const uint32_t*>(pair);
      }
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < GBK; kk += 32) {
      bf16x8 a0 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + fi][kk + fk8]);
      bf16x8 a1 = *reinterpret_cast<const bf16x8*>(
          &As[wr * 32 + 16 + fi][kk + fk8]);
      bf16x8 b0 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + fi][kk + fk8]);
      bf16x8 b1 = *reinterpret_cast<const bf16x8*>(
          &Bs[wc * 32 + 16 + fi][kk + fk8]);
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0,
                                                          acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1,
                                                          acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0,
                                                          acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1,
                                                          acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // z-partials land in per-chunk planes C[z][M][N] (plain stores; a
  // torch sum(0) folds them — measured far cheaper than 128-way fp32
  // atomic contention on every output cell).
  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
  float* Cz = C + (int64_t)blockIdx.z * plane;
#pragma unroll
  for (int fi2 = 0; fi2 < 2; ++fi2) {
#pragma unroll
    for (int fj = 0; fj < 2; ++fj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = block_row + wr * 32 + fi2 * 16 + c_row0 + r;
        const int64_t col = block_col + wc * 32 + fj * 16 + c_col;
        if (row < M && col < N) Cz[row * N + col] = acc[fi2][fj][r];
      }
    }
  }
  if (WITH_DB && blockIdx.y == 0) {
    // db[m] = sum_k A[k][m] for this block's m tile and k chunk: re-read
    // A from global (L2-hot from the staging pass just above), each
    // thread owning one (m, k-phase) stripe, then one LDS fold.
    __shared__ float dbs[GBM][4];
    const int m_l = tid & 63, phase = tid >> 6;
    float s = 0.f;
    if (block_row + m_l < M) {
      for (int64_t k = kz0 + phase; k < kz1 && k < Kb; k += 4)
        s += bf2f(A[k * M + block_row + m_l]);
    }
    dbs[m_l][phase] = s;
    __syncthreads();
    // per-chunk partial rows, plain stores into the tail of this chunk's
    // plane (db = C + M * N, planes `plane` floats apart): the host's one
    // sum(0) folds C and db together in a fixed order (atomics here made
    // db, and through Adam the whole run, differ from run to run)
    if (tid < GBM && block_row + tid < M)
      db[(int64_t)blockIdx.z * plane + block_row + tid] =
          dbs[tid][0] + dbs[tid][1] + dbs[tid][2] + dbs[tid][3];
  }
}

// ---------------------------------------------------------------------------
// 128x128 / 8-wave variant of gemm_kt: halves the A/B re-read
// amplification (traffic ∝ tiles-in-other-dim) for the big dW shapes.
// Waves as 2(m)x4(n), each wave 64x32 = 4x2 16x16 fragments.
//
// Both operands are K-major in memory (the reduction index is the row
// index), so a 64 x 128 K-step tile is staged exactly as it is loaded:
// 16-byte LDS writes of the 16-byte global loads into a [k][128] image
// with 256-byte rows, and ds_read_b64_tr_b16 turns 4-row x 16-column
// blocks of it into MFMA fragments.  No transposing write pass.
// ---------------------------------------------------------------------------
constexpr int KBM = 128, KBN = 128;
constexpr int KT_ROW_BYTES = KBM * 2;          // one k row of the image
constexpr int KT_TILE_BYTES = GBK * KT_ROW_BYTES;
static_assert(KBM == KBN, "A and B share one image geometry");

// Byte offset of 16-byte chunk `ch` (0..15) of k row `row` (0..63) in the
// tile image.  The XOR spreads both the 8-lane groups of a 16-byte store
// and the two 4-row blocks a 32-lane half reads transposed over all banks;
// stores and reads go through this one function.
__host__ __device__ constexpr int kt_tile_off(int row, int ch) {
  return KT_ROW_BYTES * row +
         16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(8))) short i16x8;

// 16x16x32 operand fragment for columns 8*c0 .. 8*c0+15 (c0 even) and
// k rows r0 .. r0+7 of this lane's 16-lane group: lane (fi, g) ends up
// with column fi, rows r0 + 0..7 in elements 0..7.  Each transposed read
// takes a 4-row block; lane 4q+p of the group addresses row q, elements
// 4p .. 4p+3 of the block.  Every lane of the wave must be active here.
__device__ __forceinline__ bf16x8 kt_frag(const unsigned char* tile, int r0,
                                          int c0, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3;
  typedef __attribute__((address_space(3))) i16x4* lds_i16x4;
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + kt_tile_off(r0 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + kt_tile_off(r0 + 4 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  return __builtin_bit_cast(
      bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// This thread's two 16-byte chunks of the K step at k0: rows
// k0 + s_row + {0, 32}, columns col0 .. col0+7 of X[Kb, ld].  kt_issue
// only starts the loads, without a branch, so that nothing waits for them
// before the MFMAs: a row past kz1 reads row kz1-1 and a chunk that is
// not wholly inside ld reads columns 0..7 instead (both in bounds: the
// chunk is not empty and ld >= 8 on this path).  kt_finish, at LDS-write
// time, zeroes what was out of range (the image is zero-padded, never
// masked) and fetches a chunk that straddles ld element by element;
// `straddle` is block-uniform and false whenever ld is a multiple of 8.
__device__ __forceinline__ void kt_issue(const __bf16* __restrict__ X,
                                         int64_t ld, int64_t col0,
                                         int64_t k0, int64_t kz1, int s_row,
                                         bf16x8 (&v)[2]) {
  const int64_t c = col0 + 7 < ld ? col0 : 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t g_k = std::min<int64_t>(k0 + s_row + 32 * h, kz1 - 1);
    v[h] = *reinterpret_cast<const bf16x8*>(&X[g_k * ld + c]);
  }
}

__device__ __forceinline__ void kt_finish(const __bf16* __restrict__ X,
                                          int64_t ld, int64_t col0,
                                          int64_t k0, int64_t kz1, int s_row,
                                          bool straddle, bf16x8 (&v)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t g_k = k0 + s_row + 32 * h;
    if (!(g_k < kz1 && col0 + 7 < ld)) v[h] = bf16x8{};
  }
  if (straddle) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t g_k = k0 + s_row + 32 * h;
      if (g_k < kz1 && col0 < ld && col0 + 7 >= ld) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col0 + e < ld) v[h][e] = X[g_k * ld + col0 + e];
      }
    }
  }
}

template <bool WITH_DB>
__global__ __launch_bounds__(512)
void gemm_kt128_kernel(const __bf16* __restrict__ A,
                       const __bf16* __restrict__ B,
                       float* __restrict__ C,
                       float* __restrict__ db,
                       int64_t Kb, int64_t M, int64_t N,
                       int64_t k_per_z, int64_t plane) {
  alignas(16) __shared__ unsigned char As[KT_TILE_BYTES];   // [k][m]
  alignas(16) __shared__ unsigned char Bs[KT_TILE_BYTES];   // [k][n]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;               // 0..7
  const int wm = wave >> 2;                // 0..1 (64 rows each)
  const int wn = wave & 3;                 // 0..3 (32 cols each)

  const int64_t block_row = (int64_t)blockIdx.x * KBM;
  const int64_t block_col = (int64_t)blockIdx.y * KBN;
  const int64_t kz0 = (int64_t)blockIdx.z * k_per_z;
  const int64_t kz1 = std::min(kz0 + k_per_z, Kb);

  f32x4b acc[4][2] = {};

  // staging: 512 threads = 32 k rows x 16 chunks, two row sets per tile
  const int s_row = tid >> 4;              // 0..31 (+32)
  const int s_ch = tid & 15;               // 16-byte chunk of the row

  const int fg8 = (lane >> 4) * 8;         // fragment k base

  // db: thread (m_l, phase) sums rows phase, phase+4, ... of column m_l
  const int m_l = tid & 127, phase = tid >> 7;
  const bool do_db = WITH_DB && blockIdx.y == 0;
  float s = 0.f;

  // the next K step's loads are in flight in registers during the MFMAs
  const int64_t a_col = block_row + s_ch * 8, b_col = block_col + s_ch * 8;
  const bool a_straddle = (M & 7) != 0 && block_row + KBM > M;
  const bool b_straddle = (N & 7) != 0 && block_col + KBN > N;
  bf16x8 va[2], vb[2];
  if (kz0 < kz1) {
    kt_issue(A, M, a_col, kz0, kz1, s_row, va);
    kt_issue(B, N, b_col, kz0, kz1, s_row, vb);
  }

  for (int64_t k0 = kz0; k0 < kz1; k0 += GBK) {
    kt_finish(A, M, a_col, k0, kz1, s_row, a_straddle, va);
    kt_finish(B, N, b_col, k0, kz1, s_row, b_straddle, vb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<bf16x8*>(
          As + kt_tile_off(s_row + 32 * h, s_ch)) = va[h];
      *reinterpret_cast<bf16x8*>(
          Bs + kt_tile_off(s_row + 32 * h, s_ch)) = vb[h];
    }
    __syncthreads();
    if (k0 + GBK < kz1) {
      kt_issue(A, M, a_col, k0 + GBK, kz1, s_row, va);
      kt_issue(B, N, b_col, k0 + GBK, kz1, s_row, vb);
    }

#pragma unroll
    for (int kk = 0; kk < GBK; kk += 32) {
      bf16x8 a[4], b[2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = kt_frag(As, kk + fg8, wm * 8 + i * 2, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = kt_frag(Bs, kk + fg8, wn * 4 + j * 2, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (do_db) {
      // from the staged tile, in ascending k; the zero rows past kz1 add
      // +0 to a sum that is never -0, so the result is that of the
      // bounded loop
#pragma unroll
      for (int r = 0; r < GBK; r += 4)
        s += bf2f(*reinterpret_cast<const __bf16*>(
            As + kt_tile_off(r + phase, m_l >> 3) + 2 * (m_l & 7)));
    }
    __syncthreads();
  }

  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
  float* Cz = C + (int64_t)blockIdx.z * plane;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = block_row + wm * 64 + i * 16 + c_row0 + r;
        const int64_t col = block_col + wn * 32 + j * 16 + c_col;
        if (row < M && col < N) Cz[row * N + col] = acc[i][j][r];
      }
    }
  }
  if (do_db) {
    __shared__ float dbs[KBM][4];
    dbs[m_l][phase] = s;
    __syncthreads();
    if (tid < KBM && block_row + tid < M)
      db[(int64_t)blockIdx.z * plane + block_row + tid] =
          dbs[tid][0] + dbs[tid][1] + dbs[tid][2] + dbs[tid][3];
  }
}

// ---------------------------------------------------------------------------
// Single-tile fragment-layout selftests.
// ---------------------------------------------------------------------------
__global__ void selftest_16x16x32(const __bf16* A, const __bf16* B,
                                  float* C) {
  const int lane = threadIdx.x;
  bf16x8 af, bf_;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    af[e] = A[(lane & 15) * 32 + (lane >> 4) * 8 + e];       // A[i][k]
    bf_[e] = B[((lane >> 4) * 8 + e) * 16 + (lane & 15)];    // B[k][j]
  }
  f32x4b acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf_, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    C[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

}  // namespace

// Rows per workgroup of the wide kernel: 64 (4 waves, 40 KB of LDS, 3
// workgroups per CU) measured faster than 128 (8 waves, 48 KB) at every
// shape and M tried.  BT_WIDE_MIN_M is the M from which the plan takes the
// wide kernel: 192 row tiles, three quarters of the 256 CUs.  Measured at
// the three call shapes of the training step: from 16.3k rows up the wide
// kernel wins at all three, at 12288 it wins one, ties one and loses one
// by 4%, and at 8192 and below the 64x64 kernel, with four times the
// workgroups, wins two of three (profiles/r06_gemm_bt_wide_kernels.md).
constexpr int WBM = 64;
constexpr int64_t BT_WIDE_MIN_M = 12288;

// Which kernel hip_gemm_bt_bf16 launches for a shape, and its grid (host
// arithmetic and two environment reads; the launcher calls it and the
// tests read it).  `aligned`: all three base pointers are 16-byte aligned.
GemmBtPlan gemm_bt_bf16_plan(int64_t M, int64_t K, int64_t N, bool aligned) {
  GemmBtPlan p;
  p.kernel = GemmBtPlan::NARROW;
  p.grid_x = (M + GBM - 1) / GBM;
  p.grid_y = (N + GBN - 1) / GBN;
  if (M <= 0 || N <= 0) return p;  // the launcher returns before it plans
  if (K <= PKP && std::getenv("GLT_GEMM_PERSIST") != nullptr) {
    p.kernel = GemmBtPlan::PERSIST;
    p.grid_x = std::min<int64_t>(p.grid_x, 1024);
    return p;
  }
  bool want = M >= BT_WIDE_MIN_M;
  if (const char* e = std::getenv("GLT_GEMM_BT")) {
    const std::string v(e);
    TORCH_CHECK(v == "wide" || v == "narrow",
                "GLT_GEMM_BT must be wide or narrow, got '", v, "'");
    want = v == "wide";
  }
  const bool can = K % 8 == 0 && K >= 32 && N >= 128 && aligned;
  if (want && can) {
    const int64_t wg = (M + WBM - 1) / WBM * ((N + WBN - 1) / WBN);
    // 1-D grid, column block fastest; beyond 2^31 - 1 workgroups (M in
    // the tens of billions) the 64x64 kernel's 2-D grid is the one left
    if (wg <= 0x7fffffff) {
      p.kernel = GemmBtPlan::WIDE;
      p.grid_x = wg;
      p.grid_y = 1;
    }
  }
  return p;
}

// Byte offset of 16-byte chunk `chunk` of row `row` in the wide kernel's
// staged [rows][64] bf16 LDS images (A: 64 rows, Bt: 256 rows; one
// function for both, the one the kernel stores and reads through).
int64_t gemm_bt_tile_offset(int64_t row, int64_t chunk) {
  TORCH_CHECK(row >= 0 && row < WBN && chunk >= 0 && chunk < GBK / 8,
              "row in [0, 256) and chunk in [0, 8) required");
  return bt_tile_off((int)row, (int)chunk);
}

// C = act(A @ Bt^T + bias): A [M,K] bf16, Bt [N,K] bf16 (nn.Linear
// weight layout), bias fp32 or none.
torch::Tensor hip_gemm_bt_bf16(const torch::Tensor& A,
                               const torch::Tensor& Bt,
                               const c10::optional<torch::Tensor>& bias,
                               bool relu, bool out_fp32) {
  TORCH_CHECK(A.is_cuda() && Bt.is_cuda(), "device tensors required");
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 &&
                  Bt.scalar_type() == torch::kBFloat16,
              "bf16 inputs required");
  TORCH_CHECK(A.dim() == 2 && Bt.dim() == 2 && A.size(1) == Bt.size(1),
              "shape mismatch");
  const int64_t M = A.size(0), K = A.size(1), N = Bt.size(0);
  auto Ac = A.contiguous();
  auto Bc = Bt.contiguous();
  auto C = torch::empty({M, N}, A.options().dtype(
                                    out_fp32 ? torch::kFloat32
                                             : torch::kBFloat16));
  if (M == 0 || N == 0) return C;  // nothing to write, no zero-dim grid
  const float* bias_p = nullptr;
  torch::Tensor bias_f;
  if (bias.has_value()) {
    bias_f = bias->to(torch::kFloat32).contiguous();
    bias_p = bias_f.data_ptr<float>();
  }
  // Dispatch (gemm_bt_bf16_plan): the wide kernel, BM x 256 tiles that
  // read A once, prefetch the next K step across the MFMAs and store
  // whole lines, wherever it applies (K % 8 == 0, K >= 32, N >= 128,
  // 16-byte aligned operands) and M is large enough to fill the CUs with
  // such tiles; the 64x64 kernel otherwise.  GLT_GEMM_BT=wide|narrow
  // overrides the M threshold only.  GLT_GEMM_PERSIST=1 (K <= 256) takes
  // precedence and selects the persistent-B experiment: whole weight
  // tile staged once, A streaming with one sync pair per m-tile.  It
  // measured SLOWER than the 64x64 kernel (L0 fwd 167 us vs 112): its
  // 68 KB of LDS halve the occupancy, and what it saves, the re-staging
  // of an L2-resident W, was never the cost; the A re-read, the missing
  // prefetch and the 2-byte stores were, and it keeps all three.
  const bool aligned =
      reinterpret_cast<uintptr_t>(Ac.data_ptr()) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(Bc.data_ptr()) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(C.data_ptr()) % 16 == 0;
  const GemmBtPlan p = gemm_bt_bf16_plan(M, K, N, aligned);
  if (p.kernel == GemmBtPlan::WIDE) {
    auto* kfn = out_fp32
                    ? (relu ? gemm_bt_wide_kernel<WBM, true, false>
                            : gemm_bt_wide_kernel<WBM, false, false>)
                    : (relu ? gemm_bt_wide_kernel<WBM, true, true>
                            : gemm_bt_wide_kernel<WBM, false, true>);
    hipLaunchKernelGGL(kfn, dim3((uint32_t)p.grid_x), dim3(WBM * 4), 0,
                       current_stream(),
                       reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                       reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                       bias_p, C.data_ptr(), M, K, N,
                       (int)((N + WBN - 1) / WBN));
    return C;
  }
  if (p.kernel == GemmBtPlan::PERSIST) {
    dim3 grid((uint32_t)p.grid_x, (uint32_t)p.grid_y);
    auto* kfn = out_fp32
                    ? (relu ? gemm_bt_persist_kernel<true, false>
                            : gemm_bt_persist_kernel<false, false>)
                    : (relu ? gemm_bt_persist_kernel<true, true>
                            : gemm_bt_persist_kernel<false, true>);
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0, current_stream(),
                       reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                       reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                       bias_p, C.data_ptr(), M, K, N);
    return C;
  }
  dim3 grid((uint32_t)p.grid_x, (uint32_t)p.grid_y);
  auto* kfn = out_fp32
                  ? (relu ? gemm_bt_kernel<true, false>
                          : gemm_bt_kernel<false, false>)
                  : (relu ? gemm_bt_kernel<true, true>
                          : gemm_bt_kernel<false, true>);
  hipLaunchKernelGGL(kfn, grid, dim3(256), 0, current_stream(),
                     reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                     reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                     bias_p, C.data_ptr(), M, K, N);
  return C;
}

// Tile size and split-K plan of hip_gemm_kt_bf16 (host arithmetic only;
// the tests read it to assert which kernel and chunking a shape reaches).
GemmKtPlan gemm_kt_bf16_plan(int64_t Kb, int64_t M, int64_t N) {
  GemmKtPlan p;
  // 128x128/8-wave tiles for big dW shapes (halves the A/B re-read
  // amplification); 64x64 for small/tail-heavy outputs
  p.big = (M >= KBM && N >= 96 && Kb >= 4096);
  const int64_t bm = p.big ? KBM : GBM, bn = p.big ? KBN : GBN;
  p.m_t = (M + bm - 1) / bm;
  p.n_t = (N + bn - 1) / bn;
  // split-K sized so the grid fills the 256 CUs a few times over
  int64_t z = 1;
  if (Kb > GBK) {
    const int64_t want_wg = p.big ? 512 : 1024;
    const int64_t tiles = std::max<int64_t>(1, p.m_t * p.n_t);
    const int64_t want = (want_wg + tiles - 1) / tiles;
    const int64_t max_z = (Kb + GBK - 1) / GBK;
    z = std::max<int64_t>(1, std::min(want, max_z));
  }
  // at least one K step, so an empty Kb still plans one (empty) chunk
  p.k_per_z =
      std::max<int64_t>(GBK, ((Kb + z - 1) / z + GBK - 1) / GBK * GBK);
  p.z = std::max<int64_t>(1, (Kb + p.k_per_z - 1) / p.k_per_z);
  return p;
}

// Byte offset of 16-byte chunk `chunk` of k row `row` in the 128x128
// kernel's [64][128] bf16 LDS tile image (the function the kernel stores
// and reads through; the tests check the layout with it, without a GPU).
int64_t gemm_kt_tile_offset(int64_t row, int64_t chunk) {
  TORCH_CHECK(row >= 0 && row < GBK && chunk >= 0 && chunk < KBM / 8,
              "row in [0, 64) and chunk in [0, 16) required");
  return kt_tile_off((int)row, (int)chunk);
}

// (dW, db) = (A^T @ B, colsum(A)): A [Kb,M] bf16, B [Kb,N] bf16;
// outputs fp32 (master-grad dtype).  with_db=false skips db.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> hip_gemm_kt_bf16(
    const torch::Tensor& A, const torch::Tensor& B, bool with_db) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "device tensors required");
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 &&
                  B.scalar_type() == torch::kBFloat16,
              "bf16 inputs required");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(0) == B.size(0),
              "shape mismatch");
  const int64_t Kb = A.size(0), M = A.size(1), N = B.size(1);
  c10::optional<torch::Tensor> db;
  float* db_p = nullptr;
  // empty reduction or empty output: zeros, before any plan arithmetic
  // or launch (a grid dimension of 0 is a launch error)
  if (Kb == 0 || M == 0 || N == 0) {
    // db = colsum(A) does not depend on N: with an empty dW it is the
    // only output left, zeros when the reduction itself is empty
    if (with_db) db = A.sum({0}, /*keepdim=*/false, torch::kFloat32);
    return {torch::zeros({M, N}, A.options().dtype(torch::kFloat32)), db};
  }
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  const GemmKtPlan p = gemm_kt_bf16_plan(Kb, M, N);
  const bool big = p.big;
  const int64_t m_t = p.m_t, n_t = p.n_t, z = p.z, k_per_z = p.k_per_z;
  // z>1: per-chunk partial planes + one sum(0) (no output atomics).  A
  // plane is C's [M, N] followed, with_db, by the chunk's db row [M]:
  // every (chunk, m) db cell is stored exactly once, by the
  // blockIdx.y == 0 block of that (m tile, chunk).
  const int64_t plane = M * N + (with_db ? M : 0);
  auto P = torch::empty({z, plane}, A.options().dtype(torch::kFloat32));
  if (with_db) db_p = P.data_ptr<float>() + M * N;
  dim3 grid((uint32_t)m_t, (uint32_t)n_t, (uint32_t)z);
  if (big) {
    auto* kfn = with_db ? gemm_kt128_kernel<true>
                        : gemm_kt128_kernel<false>;
    hipLaunchKernelGGL(kfn, grid, dim3(512), 0, current_stream(),
                       reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                       reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                       P.data_ptr<float>(), db_p, Kb, M, N, k_per_z,
                       plane);
  } else {
    auto* kfn = with_db ? gemm_kt_kernel<true> : gemm_kt_kernel<false>;
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0, current_stream(),
                       reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                       reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                       P.data_ptr<float>(), db_p, Kb, M, N, k_per_z,
                       plane);
  }
  auto flat = z == 1 ? P.squeeze(0) : P.sum(0);
  if (with_db) db = flat.narrow(0, M * N, M);
  return {flat.narrow(0, 0, M * N).view({M, N}), db};
}

torch::Tensor hip_mfma_bf16_selftest(const torch::Tensor& A,
                                     const torch::Tensor& B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
              B.sizes() == torch::IntArrayRef({32, 16}),
              "selftest is 16x32 @ 32x16");
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  auto C = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(selftest_16x16x32, dim3(1), dim3(64), 0,
                     current_stream(),
                     reinterpret_cast<const __bf16*>(Ac.data_ptr()),
                     reinterpret_cast<const __bf16*>(Bc.data_ptr()),
                     C.data_ptr<float>());
  return C;
}

}  // namespace glt

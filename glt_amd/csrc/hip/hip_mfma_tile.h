/* Staged-as-loaded LDS tile images for the 16x16x32_bf16 MFMA GEMMs that
 * prefetch (hip_gemm_bf16.hip: gemm_bt_wide_kernel, gemm_kt128_kernel;
 * hip_gemm_grouped.hip: relation_gemm_kernel, relation_wgrad_kernel).
 * Everything here is parameterised by tile dimensions and operands; the
 * kernels keep their work decode, their bias rule and their LDS.
 *
 * Fragment layout (cdna4 §10): A lane l holds A[i=l&15][k=(l>>4)*8+e], B
 * lane l holds B[k=(l>>4)*8+e][j=l&15], C/D col=l&15, row=(l>>4)*4+reg.
 *
 *  rm_*: operands K-innermost in memory (A [M, K], Bt [N, K]), staged into
 *        [row][64] images with 128-byte rows, 16-byte fragment reads.
 *  km_*: operands K-major in memory (A [Kb, M], B [Kb, N]), staged into
 *        [k][128] images with 256-byte rows, fragments built by the
 *        transposed LDS read ds_read_b64_tr_b16.
 *
 * In both, the 16-byte global loads of K step i+1 are issued into registers
 * right after the barrier of step i, before its MFMAs, and written to LDS,
 * 16 bytes at a time, after them.  The loads are issued without a branch (a
 * divergent branch around a load makes the compiler wait for it at the
 * join, ahead of the MFMAs): an out-of-range row or chunk reads an in-range
 * address and is zeroed at LDS-write time.  The images are zero-padded,
 * MFMA lanes are never masked.  Index width I is the caller's (int64_t in
 * the dense kernels, int in the grouped ones).
 *
 * No packed fp32 arithmetic: the functions here switch that target feature
 * off for themselves, wherever the header is included, and a kernel built
 * from them carries GLT_NO_PACKED_FP32 (or lies in a file-wide pragma of
 * the same kind), so that caller and callee have one feature set.  For the
 * same reason nothing here calls a library function that is not forced
 * inline (std::min): declared under other features, it would stay a call.
 */
#pragma once

#include "hip_common.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define GLT_NO_PACKED_FP32 __attribute__((target("no-packed-fp32-ops")))
#pragma clang attribute push(GLT_NO_PACKED_FP32, apply_to = function)
#else
#define GLT_NO_PACKED_FP32
#endif

namespace glt {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) short i16x4;

constexpr int MT_BK = 64;                  // K step of every image

// __syncthreads(), written out: the runtime header's is not forced inline
// either and would stay a call from a function compiled under this pragma.
__device__ __forceinline__ void tile_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---------------------------------------------------------------------------
// Row-major image: [row][64] bf16, 128-byte rows.
// ---------------------------------------------------------------------------
constexpr int RM_ROW_BYTES = MT_BK * 2;    // one staged row: 64 k
constexpr int RM_EP_LD = 68;               // epilogue row stride in floats

// Byte offset of 16-byte chunk `ch` (0..7: k = 8 ch .. 8 ch + 7) of row
// `row` in a staged image.  Rows are 128 bytes, so two rows fill the 64
// banks once; XOR-ing the chunk with bits 1..3 of the row makes the eight
// rows of one parity in any aligned 16-row block start in eight different
// 16-byte slots.  The 8 lanes of a 16-byte store group write the 8 chunks
// of one row (a permutation of the 8 slots), and the 16 lanes of a
// 16-byte read group, 8 rows at chunk c and 8 at chunk c ^ 1 of one
// aligned 16-row block, cover all 64 banks exactly once.
__host__ __device__ constexpr int rm_tile_off(int row, int ch) {
  return RM_ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

// This thread's 16-byte chunks of the K step at k0: chunk s_ch of rows
// row0 + s_row + RPP * h of X[rows, K] (row stride ld).  rm_issue only
// starts the loads: a row past `rows` reads the last row and a chunk past
// K reads chunk 0 (both in bounds: rows >= 1, K >= 8 and K % 8 == 0 on
// these paths, so a chunk is wholly inside K or wholly outside).
// rm_finish, at LDS-write time, zeroes what was out of range.
template <int NV, int RPP, typename I>
__device__ __forceinline__ void rm_issue(const __bf16* __restrict__ X, I rows,
                                         I K, int64_t ld, I row0, I k0,
                                         int s_row, int s_ch,
                                         bf16x8 (&v)[NV]) {
  const I k = k0 + s_ch * 8;
  const I kc = k + 8 <= K ? k : 0;
#pragma unroll
  for (int h = 0; h < NV; ++h) {
    const I row = row0 + s_row + RPP * h;
    const I g_row = row < rows ? row : rows - 1;
    v[h] = *reinterpret_cast<const bf16x8*>(&X[(int64_t)g_row * ld + kc]);
  }
}

template <int NV, int RPP, typename I>
__device__ __forceinline__ void rm_finish(I rows, I K, I row0, I k0,
                                          int s_row, int s_ch,
                                          bf16x8 (&v)[NV]) {
  const bool k_in = k0 + s_ch * 8 + 8 <= K;
#pragma unroll
  for (int h = 0; h < NV; ++h)
    if (!(k_in && row0 + s_row + RPP * h < rows)) v[h] = bf16x8{};
}

// acc += A[block_row .., :K] @ Bt[block_col .., :K]^T for a BM x BN
// workgroup tile, (BM / 16 MI) x (BN / 16 NJ) waves, each wave MI x NJ
// fragments.  smem holds the A image, then the Bt image; every wave leaves
// past a barrier, so the caller may reuse it (another operand pair, or
// rm_store_lines).  8 lanes stage the 8 chunks of one row.  Lane group g
// holds k = kk + 8g .. +7 and kk ascends; a kk step of nothing but zero
// padding is skipped (it would add +0), and a wave whose columns all lie
// past N multiplies nothing.
template <int BM, int BN, int MI, int NJ, typename I>
__device__ __forceinline__ void rm_k_loop(unsigned char* smem,
                                          const __bf16* __restrict__ A,
                                          int64_t lda, I M,
                                          const __bf16* __restrict__ Bt, I N,
                                          I K, I block_row, I block_col,
                                          f32x4 (&acc)[MI][NJ]) {
  constexpr int WN = BN / (16 * NJ);       // waves along the columns
  constexpr int NT = BM / (16 * MI) * WN * 64;
  constexpr int RPP = NT / 8;              // rows one staging pass covers
  constexpr int NA = BM / RPP, NB = BN / RPP;
  static_assert(BM % (16 * MI) == 0 && BN % (16 * NJ) == 0 && NA >= 1 &&
                    NB >= 1, "whole wave tiles and staging passes");
  static_assert((NT / 64) * 16 * RM_EP_LD * 4 <= (BM + BN) * RM_ROW_BYTES,
                "epilogue tiles fit in the staging buffers");
  if (K <= 0) return;
  unsigned char* const As = smem;
  unsigned char* const Bs = smem + BM * RM_ROW_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const bool live = block_col + wn * (16 * NJ) < N;
  const int s_row = tid >> 3;
  const int s_ch = tid & 7;
  const int fi = lane & 15;                // fragment row / col
  const int fg = lane >> 4;                // fragment k group

  bf16x8 va[NA], vb[NB];
  rm_issue<NA, RPP>(A, M, K, lda, block_row, I(0), s_row, s_ch, va);
  rm_issue<NB, RPP>(Bt, N, K, (int64_t)K, block_col, I(0), s_row, s_ch, vb);

  for (I k0 = 0; k0 < K; k0 += MT_BK) {
    rm_finish<NA, RPP>(M, K, block_row, k0, s_row, s_ch, va);
    rm_finish<NB, RPP>(N, K, block_col, k0, s_row, s_ch, vb);
#pragma unroll
    for (int h = 0; h < NA; ++h)
      *reinterpret_cast<bf16x8*>(
          As + rm_tile_off(s_row + RPP * h, s_ch)) = va[h];
#pragma unroll
    for (int h = 0; h < NB; ++h)
      *reinterpret_cast<bf16x8*>(
          Bs + rm_tile_off(s_row + RPP * h, s_ch)) = vb[h];
    tile_barrier();
    if (k0 + MT_BK < K) {
      rm_issue<NA, RPP>(A, M, K, lda, block_row, k0 + MT_BK, s_row, s_ch, va);
      rm_issue<NB, RPP>(Bt, N, K, (int64_t)K, block_col, k0 + MT_BK, s_row,
                        s_ch, vb);
    }
#pragma unroll
    for (int kk = 0; kk < MT_BK; kk += 32) {
      // a kk step past K holds only zero padding
      if (live && k0 + kk < K) {
        bf16x8 a[MI], b[NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
          a[i] = *reinterpret_cast<const bf16x8*>(
              As + rm_tile_off(wm * (16 * MI) + i * 16 + fi, (kk >> 3) + fg));
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          b[j] = *reinterpret_cast<const bf16x8*>(
              Bs + rm_tile_off(wn * (16 * NJ) + j * 16 + fi, (kk >> 3) + fg));
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    tile_barrier();
  }
}

// Epilogue of a wave's MI x NJ accumulator tile whose first cell is
// (wave_row, wave_col) of C[M, N].  With add_bias, col_bias[j] (this lane's
// bias of column wave_col + 16 j + (lane & 15)) is added in fp32 on every
// row, here and not by the caller: an addition into the accumulators ahead
// of this function costs a round trip through the AGPRs, measured at 2% of
// the wide kernel.  A bias that does not cover every row is the caller's
// to add first.  ReLU, then the wave passes the tile, 16 rows at a time,
// through its own [16][68] fp32 LDS tile (the staging buffers: every wave
// is past the last barrier of rm_k_loop) and writes whole row pieces, 16
// bytes per lane: 8 lanes a 128-byte row piece of bf16 (rounded once,
// here), 16 lanes 256 bytes of fp32.  The 68-float stride puts the two rows a 32-lane half
// writes 16 banks apart.  A row of C starts 16-byte aligned only if N is a
// multiple of 8 (bf16) or 4 (fp32); otherwise, and in the N tail, elements
// are stored one by one.
template <int MI, int NJ, bool BF16_OUT, typename I>
__device__ __forceinline__ void rm_store_lines(unsigned char* smem,
                                               const f32x4 (&acc)[MI][NJ],
                                               const float (&col_bias)[NJ],
                                               bool add_bias, bool relu,
                                               void* __restrict__ Cv, I M,
                                               I N, I wave_row, I wave_col) {
  static_assert(NJ == 4, "the LDS tile and the lane maps are 64 columns");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  float* const ep = reinterpret_cast<float*>(smem) + wave * (16 * RM_EP_LD);
  constexpr int CPL = BF16_OUT ? 8 : 4;    // columns per lane
  constexpr int LPR = 64 / CPL;            // lanes per 64-column row piece
  constexpr int RPI = 64 / LPR;            // rows per wave instruction
  const bool vec_ok = N % CPL == 0;
  const int e_row = lane / LPR;
  const int e_col = (lane % LPR) * CPL;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r];
        if (add_bias) v += col_bias[j];
        if (relu) v = v > 0.f ? v : 0.f;
        ep[(fg * 4 + r) * RM_EP_LD + j * 16 + fi] = v;
      }
    }
    tile_barrier();
#pragma unroll
    for (int h = 0; h < 16 / RPI; ++h) {
      const int rr = e_row + RPI * h;
      const I row = wave_row + i * 16 + rr;
      const I col = wave_col + e_col;
      const float* src = ep + rr * RM_EP_LD + e_col;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(src);
      if (BF16_OUT) {
        const f32x4 hi = *reinterpret_cast<const f32x4*>(src + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (__bf16)lo[e];
          o[4 + e] = (__bf16)hi[e];
        }
        __bf16* dst = reinterpret_cast<__bf16*>(Cv) + (int64_t)row * N + col;
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
        float* dst = reinterpret_cast<float*>(Cv) + (int64_t)row * N + col;
        if (row < M) {
          if (vec_ok && col + 3 < N) {
            *reinterpret_cast<f32x4*>(dst) = lo;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < N) dst[e] = lo[e];
          }
        }
      }
    }
    tile_barrier();
  }
}

// ---------------------------------------------------------------------------
// K-major image: [k][128] bf16, 256-byte rows; 128 x 128 tile, 8 waves as
// 2 (m) x 4 (n), each wave 64 x 32 = 4 x 2 fragments.  512 threads = 32 k
// rows x 16 chunks, two row sets per K step.
// ---------------------------------------------------------------------------
constexpr int KM_BT = 128;                     // tile edge
constexpr int KM_ROW_BYTES = KM_BT * 2;        // one k row of the image
constexpr int KM_TILE_BYTES = MT_BK * KM_ROW_BYTES;

// Byte offset of 16-byte chunk `ch` (0..15) of k row `row` (0..63) in the
// tile image.  The XOR spreads both the 8-lane groups of a 16-byte store
// and the two 4-row blocks a 32-lane half reads transposed over all banks;
// stores and reads go through this one function.
__host__ __device__ constexpr int km_tile_off(int row, int ch) {
  return KM_ROW_BYTES * row +
         16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// 16x16x32 operand fragment for columns 8*c0 .. 8*c0+15 (c0 even) and
// k rows r0 .. r0+7 of this lane's 16-lane group: lane (fi, g) ends up
// with column fi, rows r0 + 0..7 in elements 0..7.  Each transposed read
// takes a 4-row block; lane 4q+p of the group addresses row q, elements
// 4p .. 4p+3 of the block.  Every lane of the wave must be active here.
__device__ __forceinline__ bf16x8 km_frag(const unsigned char* tile, int r0,
                                          int c0, int lane) {
  const int q = (lane & 15) >> 2, p = lane & 3;
  typedef __attribute__((address_space(3))) i16x4* lds_i16x4;
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + km_tile_off(r0 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4)(
      tile + km_tile_off(r0 + 4 + q, c0 + (p >> 1)) + 8 * (p & 1)));
  return __builtin_bit_cast(
      bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// This thread's two 16-byte chunks of the K step at k0: rows
// k0 + s_row + {0, 32}, columns col0 .. col0+7 of X[., cols] (row stride
// ld).  km_issue only starts the loads: a row past kz1 reads row kz1-1 and
// a chunk that is not wholly inside cols reads columns 0..7 instead (both
// in bounds: the k range is not empty and cols >= 8 on these paths).
// km_finish, at LDS-write time, zeroes what was out of range and fetches a
// chunk that straddles cols element by element; `straddle` is
// block-uniform and false whenever cols is a multiple of 8.
template <typename I>
__device__ __forceinline__ void km_issue(const __bf16* __restrict__ X,
                                         int64_t ld, I cols, I col0, I k0,
                                         I kz1, int s_row, bf16x8 (&v)[2]) {
  const I c = col0 + 8 <= cols ? col0 : 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const I row = k0 + s_row + 32 * h;
    const I g_k = row < kz1 ? row : kz1 - 1;
    v[h] = *reinterpret_cast<const bf16x8*>(&X[(int64_t)g_k * ld + c]);
  }
}

template <typename I>
__device__ __forceinline__ void km_finish(const __bf16* __restrict__ X,
                                          int64_t ld, I cols, I col0, I k0,
                                          I kz1, int s_row, bool straddle,
                                          bf16x8 (&v)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const I g_k = k0 + s_row + 32 * h;
    if (!(g_k < kz1 && col0 + 8 <= cols)) v[h] = bf16x8{};
  }
  if (straddle) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const I g_k = k0 + s_row + 32 * h;
      if (g_k < kz1 && col0 < cols && col0 + 8 > cols) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col0 + e < cols) v[h][e] = X[(int64_t)g_k * ld + col0 + e];
      }
    }
  }
}

// acc += A[kz0 .. kz1, block_row ..]^T @ B[kz0 .. kz1, block_col ..] over
// the images As, Bs (KM_TILE_BYTES each).  With do_db, thread (m_l, phase)
// = (tid & 127, tid >> 7) also adds rows phase, phase+4, ... of column m_l
// of every staged A tile to dsum, in ascending k; the zero rows past kz1
// add +0 to a sum that is never -0, so the result is that of a bounded
// loop.  Every wave leaves past a barrier.
template <typename I>
__device__ __forceinline__ void km_k_loop(
    unsigned char* As, unsigned char* Bs, const __bf16* __restrict__ A,
    int64_t lda, I a_cols, bool a_straddle, const __bf16* __restrict__ B,
    int64_t ldb, I b_cols, bool b_straddle, I block_row, I block_col, I kz0,
    I kz1, bool do_db, f32x4 (&acc)[4][2], float& dsum) {
  if (kz0 >= kz1) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 2;                // 64 rows each
  const int wn = wave & 3;                 // 32 cols each
  const int s_row = tid >> 4;              // 0..31 (+32)
  const int s_ch = tid & 15;               // 16-byte chunk of the row
  const int fg8 = (lane >> 4) * 8;         // fragment k base
  const int m_l = tid & 127, phase = tid >> 7;

  const I a_col = block_row + s_ch * 8, b_col = block_col + s_ch * 8;
  bf16x8 va[2], vb[2];
  km_issue(A, lda, a_cols, a_col, kz0, kz1, s_row, va);
  km_issue(B, ldb, b_cols, b_col, kz0, kz1, s_row, vb);

  for (I k0 = kz0; k0 < kz1; k0 += MT_BK) {
    km_finish(A, lda, a_cols, a_col, k0, kz1, s_row, a_straddle, va);
    km_finish(B, ldb, b_cols, b_col, k0, kz1, s_row, b_straddle, vb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<bf16x8*>(
          As + km_tile_off(s_row + 32 * h, s_ch)) = va[h];
      *reinterpret_cast<bf16x8*>(
          Bs + km_tile_off(s_row + 32 * h, s_ch)) = vb[h];
    }
    tile_barrier();
    if (k0 + MT_BK < kz1) {
      km_issue(A, lda, a_cols, a_col, k0 + MT_BK, kz1, s_row, va);
      km_issue(B, ldb, b_cols, b_col, k0 + MT_BK, kz1, s_row, vb);
    }
#pragma unroll
    for (int kk = 0; kk < MT_BK; kk += 32) {
      bf16x8 a[4], b[2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a[i] = km_frag(As, kk + fg8, wm * 8 + i * 2, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j] = km_frag(Bs, kk + fg8, wn * 4 + j * 2, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (do_db) {
#pragma unroll
      for (int r = 0; r < MT_BK; r += 4)
        dsum += (float)*reinterpret_cast<const __bf16*>(
            As + km_tile_off(r + phase, m_l >> 3) + 2 * (m_l & 7));
    }
    tile_barrier();
  }
}

// The tile's cells of this chunk's fp32 plane Cz[M, N], plain stores (a
// later fold adds the chunks in a fixed order; output atomics measured
// contention-bound and made db differ from run to run).  With do_db the
// four phase sums of km_k_loop are folded through dbs and the tile's part
// of the chunk's db row dbz[M] is stored, every cell exactly once.
template <typename I>
__device__ __forceinline__ void km_store_plane(
    float* __restrict__ Cz, float* __restrict__ dbz, float (&dbs)[KM_BT][4],
    I M, I N, I block_row, I block_col, const f32x4 (&acc)[4][2], bool do_db,
    float dsum) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const I row = block_row + wm * 64 + i * 16 + c_row0 + r;
        const I col = block_col + wn * 32 + j * 16 + c_col;
        if (row < M && col < N) Cz[(int64_t)row * N + col] = acc[i][j][r];
      }
    }
  }
  if (do_db) {
    dbs[tid & 127][tid >> 7] = dsum;
    tile_barrier();
    if (tid < KM_BT && block_row + tid < M)
      dbz[block_row + tid] =
          dbs[tid][0] + dbs[tid][1] + dbs[tid][2] + dbs[tid][3];
  }
}

}  // namespace glt

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

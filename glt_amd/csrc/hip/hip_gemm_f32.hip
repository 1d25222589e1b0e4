/* Hand-written f32 MFMA GEMM for GNN projection shapes (gfx950).
 *
 * C[m,n] = A[m,k] @ B[k,n] (+ bias), fp32 in / fp32 out, exact f32
 * numerics via v_mfma_f32_16x16x4_f32 (the CDNA4 "SGEMM" matrix-core op:
 * 157 TF chip peak = 16x the rocBLAS pick we measured on these shapes —
 * tall-skinny m~1e5, n=256, k=200/512 batches where Tensile chooses
 * MT32x32 tiles at ~51 TF).
 *
 * Geometry: 64x64 block tile, 4 waves as 2x2, each wave a 32x32 tile of
 * four 16x16 fragments (4 independent accumulators: the 16x16x4 form needs
 * >=2 for back-to-back issue, guide §3).  K staged through LDS in BK=16
 * steps with +1-row padding (bank-conflict rule, guide §6 G4); edge tiles
 * (m tail, k tail) zero-filled so no host-side padding is needed.
 */
#include "hip_common.h"
#include "../include/common.h"

namespace glt {

namespace {

using f32x4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;

constexpr int BM = 64, BN = 64;

template <int BK, bool RELU>
__global__ __launch_bounds__(256)
void sage_gemm_f32_kernel(const float* __restrict__ A,
                          const float* __restrict__ B,
                          const float* __restrict__ bias,
                          float* __restrict__ C,
                          int64_t M, int64_t K, int64_t N) {
  __shared__ float As[BM][BK + 1];
  __shared__ float Bs[BK][BN + 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;          // 0..3
  const int wr = wave >> 1;           // wave row (32 rows each)
  const int wc = wave & 1;            // wave col (32 cols each)

  const int64_t block_row = (int64_t)blockIdx.x * BM;
  const int64_t block_col = (int64_t)blockIdx.y * BN;

  f32x4 acc[2][2] = {};  // 2x2 fragments of 16x16

  const int frag_i = lane & 15;
  const int frag_k = lane >> 4;

  for (int64_t k0 = 0; k0 < K; k0 += BK) {
    const int64_t kmax = K - k0;
    // stage A tile [BM][BK] as float4s, grid-stride over the tile
#pragma unroll
    for (int idx = 0; idx < BM * BK / 4 / 256; ++idx) {
      const int e = tid + idx * 256;
      const int row = e / (BK / 4);
      const int col = (e % (BK / 4)) * 4;
      const int64_t g_row = block_row + row;
      float4 f = {0.f, 0.f, 0.f, 0.f};
      if (g_row < M) {
        const int64_t base = g_row * K + k0 + col;
        if (col + 3 < kmax) {
          f = *reinterpret_cast<const float4*>(&A[base]);
        } else {
          if (col + 0 < kmax) f.x = A[base + 0];
          if (col + 1 < kmax) f.y = A[base + 1];
          if (col + 2 < kmax) f.z = A[base + 2];
          if (col + 3 < kmax) f.w = A[base + 3];
        }
      }
      As[row][col + 0] = f.x;
      As[row][col + 1] = f.y;
      As[row][col + 2] = f.z;
      As[row][col + 3] = f.w;
    }
    // stage B tile [BK][BN]
#pragma unroll
    for (int idx = 0; idx < BK * BN / 4 / 256; ++idx) {
      const int e = tid + idx * 256;
      const int row = e / (BN / 4);
      const int col = (e % (BN / 4)) * 4;
      const int64_t g_k = k0 + row;
      float4 f = {0.f, 0.f, 0.f, 0.f};
      if (g_k < K) {
        f = *reinterpret_cast<const float4*>(
            &B[g_k * N + block_col + col]);
      }
      Bs[row][col + 0] = f.x;
      Bs[row][col + 1] = f.y;
      Bs[row][col + 2] = f.z;
      Bs[row][col + 3] = f.w;
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float a0 = As[wr * 32 + frag_i][kk + frag_k];
      float a1 = As[wr * 32 + 16 + frag_i][kk + frag_k];
      float b0 = Bs[kk + frag_k][wc * 32 + frag_i];
      float b1 = Bs[kk + frag_k][wc * 32 + 16 + frag_i];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0],
                                                       0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1],
                                                       0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0],
                                                       0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1],
                                                       0, 0, 0);
    }
    __syncthreads();
  }

  // C/D layout for 16x16x4f32: col = lane&15, row = (lane>>4)*4 + reg.
  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
#pragma unroll
    for (int fj = 0; fj < 2; ++fj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = block_row + wr * 32 + fi * 16 + c_row0 + r;
        const int64_t col = block_col + wc * 32 + fj * 16 + c_col;
        if (row < M) {
          float v = acc[fi][fj][r];
          if (bias != nullptr) v += bias[col];
          if (RELU) v = v > 0.f ? v : 0.f;
          C[row * N + col] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 128x128x32 variant on v_mfma_f32_32x32x2_f32 (16 accumulators/frag,
// 64-cycle issue = dependent latency, guide §3): 4 waves as 2x2, each wave
// a 64x64 tile of 2x2 32x32 fragments.  The geometry the CDNA4 guide
// measures at 122 TF untuned for f32.
// ---------------------------------------------------------------------------
using f32x16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;

constexpr int BM2 = 128, BN2 = 128, BK2 = 32;

template <bool RELU>
__global__ __launch_bounds__(256)
void sage_gemm_f32_128_kernel(const float* __restrict__ A,
                              const float* __restrict__ B,
                              const float* __restrict__ bias,
                              float* __restrict__ C,
                              int64_t M, int64_t K, int64_t N) {
  __shared__ float As[BM2][BK2 + 1];
  __shared__ float Bs[BK2][BN2 + 1];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;           // 0..1, 64 rows each
  const int wc = wave & 1;            // 0..1, 64 cols each

  const int64_t block_row = (int64_t)blockIdx.x * BM2;
  const int64_t block_col = (int64_t)blockIdx.y * BN2;

  f32x16 acc[2][2] = {};

  // staging: A tile 128x32 floats = 4096 -> 16 per thread as 4x float4
  // thread t loads A rows (t>>2)*? : layout: 8 rows per 32-thread group.
  const int a_row0 = tid >> 1;         // 0..127, each thread 1 row half
  const int a_col8 = (tid & 1) * 16;   // two threads cover 32 floats/row
  const int b_row0 = tid >> 3;         // 0..31
  const int b_col16 = (tid & 7) * 16;  // 8 threads cover 128 floats/row

  const int fi_row = lane & 31;        // A fragment row
  const int fk = lane >> 5;            // k sub-lane 0..1

  for (int64_t k0 = 0; k0 < K; k0 += BK2) {
    // stage A: each thread 16 floats of one row (4x float4)
    {
      const int64_t g_row = block_row + a_row0;
      const int64_t kmax = K - k0;
#pragma unroll
      for (int c = 0; c < 16; c += 4) {
        const int col = a_col8 + c;
        float4 f = {0.f, 0.f, 0.f, 0.f};
        if (g_row < M) {
          const int64_t base = g_row * K + k0 + col;
          if (col + 3 < kmax) {
            f = *reinterpret_cast<const float4*>(&A[base]);
          } else {
            if (col + 0 < kmax) f.x = A[base + 0];
            if (col + 1 < kmax) f.y = A[base + 1];
            if (col + 2 < kmax) f.z = A[base + 2];
            if (col + 3 < kmax) f.w = A[base + 3];
          }
        }
        As[a_row0][col + 0] = f.x;
        As[a_row0][col + 1] = f.y;
        As[a_row0][col + 2] = f.z;
        As[a_row0][col + 3] = f.w;
      }
    }
    // stage B: each thread 16 floats of one k-row
    {
      const int64_t g_k = k0 + b_row0;
#pragma unroll
      for (int c = 0; c < 16; c += 4) {
        const int col = b_col16 + c;
        float4 f = {0.f, 0.f, 0.f, 0.f};
        if (g_k < K) {
          f = *reinterpret_cast<const float4*>(
              &B[g_k * N + block_col + col]);
        }
        Bs[b_row0][col + 0] = f.x;
        Bs[b_row0][col + 1] = f.y;
        Bs[b_row0][col + 2] = f.z;
        Bs[b_row0][col + 3] = f.w;
      }
    }
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < BK2; kk += 2) {
      const float a0 = As[wr * 64 + fi_row][kk + fk];
      const float a1 = As[wr * 64 + 32 + fi_row][kk + fk];
      const float b0 = Bs[kk + fk][wc * 64 + fi_row];
      const float b1 = Bs[kk + fk][wc * 64 + 32 + fi_row];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0],
                                                       0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1],
                                                       0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0],
                                                       0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1],
                                                       0, 0, 0);
    }
    __syncthreads();
  }

  // C layout for 32x32x2f32: col = lane&31, row = (reg&3) + 8*(reg>>2)
  // + 4*(lane>>5)  (guide §3).
  const int c_col = lane & 31;
  const int c_rbase = 4 * (lane >> 5);
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
#pragma unroll
    for (int fj = 0; fj < 2; ++fj) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row_in = (reg & 3) + 8 * (reg >> 2) + c_rbase;
        const int64_t row = block_row + wr * 64 + fi * 32 + row_in;
        const int64_t col = block_col + wc * 64 + fj * 32 + c_col;
        if (row < M) {
          float v = acc[fi][fj][reg];
          if (bias != nullptr) v += bias[col];
          if (RELU) v = v > 0.f ? v : 0.f;
          C[row * N + col] = v;
        }
      }
    }
  }
}

}  // namespace

// C = A @ B (+bias). A [M,K] row-major, B [K,N] row-major; N % 64 == 0.
torch::Tensor hip_sage_gemm(const torch::Tensor& A, const torch::Tensor& B,
                            const c10::optional<torch::Tensor>& bias,
                            bool relu) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "device tensors required");
  TORCH_CHECK(A.scalar_type() == torch::kFloat32 &&
              B.scalar_type() == torch::kFloat32, "fp32 only");
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && A.size(1) == B.size(0));
  const int64_t M = A.size(0), K = A.size(1), N = B.size(1);
  TORCH_CHECK(N % 64 == 0, "N must be a multiple of 64");
  auto Ac = A.contiguous();
  auto Bc = B.contiguous();
  auto C = torch::empty({M, N}, A.options());
  if (M == 0 || N == 0) return C;  // nothing to write, no zero-dim grid
  const float* bias_p =
      bias.has_value() ? bias->data_ptr<float>() : nullptr;
  // the 128x128 tile pays only with enough K depth to amortize its
  // staging; skinny-K projection shapes stay on the 64x64xBK64 kernel
  if (N % BN2 == 0 && M >= BM2 && K >= 384) {
    dim3 grid((uint32_t)((M + BM2 - 1) / BM2), (uint32_t)(N / BN2));
    auto* kfn = relu ? sage_gemm_f32_128_kernel<true>
                     : sage_gemm_f32_128_kernel<false>;
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0,
                       current_stream(), Ac.data_ptr<float>(),
                       Bc.data_ptr<float>(), bias_p, C.data_ptr<float>(),
                       M, K, N);
  } else {
    dim3 grid((uint32_t)((M + BM - 1) / BM), (uint32_t)(N / BN));
    auto* kfn = relu ? sage_gemm_f32_kernel<16, true>
                     : sage_gemm_f32_kernel<16, false>;
    hipLaunchKernelGGL(kfn, grid, dim3(256), 0,
                       current_stream(), Ac.data_ptr<float>(),
                       Bc.data_ptr<float>(), bias_p, C.data_ptr<float>(),
                       M, K, N);
  }
  return C;
}

}  // namespace glt

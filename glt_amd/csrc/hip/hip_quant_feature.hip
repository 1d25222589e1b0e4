/* 8-bit feature rows: row quantiser and gather-dequantise (gfx950).
 *
 * Packed row format (one definition; ops/quant.py is its torch twin): a table
 * is uint8 [N, S], S = round_up(F + 4, 16).  Row r holds F codes in bytes
 * [0, F), zero padding in [F, S - 4) and the row's fp32 scale, little endian,
 * in [S - 4, S).  The scale is inline so a cold-tier row is one contiguous
 * PCIe read; every row is 16-byte aligned.  Codes are symmetric int8 in
 * [-127, 127] or OCP e4m3 (torch.float8_e4m3fn, |max| 448).
 *
 * Quantising a row x[0..F), every line one rounded fp32 operation:
 *   amax  = max |x[f]|                       (NaN counts as 0)
 *   amax < 2^-119 or inf: scale = 0, codes 0
 *   scale = amax / QMAX;  inv = QMAX / amax
 *   y[f]  = clamp(x[f] * inv, -QMAX, QMAX)   (NaN -> 0)
 *   int8: rintf(y[f]);  fp8: y[f] rounded to e4m3, nearest even
 * Dequantising is float(code) * scale, then one RNE rounding for bf16.
 *
 * quantize_rows_kernel: one wave per row, lane l owns channels 4l .. 4l + 3
 * of every pass of 256 channels and the 4-byte code word they make.  A row
 * of up to 256 channels stays in registers between the absmax pass and the
 * code pass; a wider one is read twice.  The words past the codes are the
 * zero padding, so the code pass writes every byte of the row but the scale,
 * which lane 0 stores.
 *
 * gather_dequant_kernel: element-level like gather_rows_kernel.  A thread
 * owns one chunk of 16 output bytes (8 bf16 or 4 fp32 values) of one output
 * row: one 8- or 4-byte load of codes, the row's scale from its last four
 * bytes, one 16-byte store.  Output rows are F elements wide without
 * padding, so where F elements are no multiple of 16 bytes the launcher
 * picks the widest store (8, 4 or 2 bytes) that every row start is aligned
 * to and a chunk goes out in 16 / VS pieces, the pieces past the row
 * dropped.  The choice is made once per launch, not per lane.
 */
#include "hip_common.h"
#include "hip_seg_table.h"
#include "hip_wave.h"
#include "../include/hip_ops.h"

#include <cfloat>

// the definition has no fused operations
#pragma clang fp contract(off)

namespace glt {

namespace {

enum QFmt { kInt8 = 0, kFp8 = 1 };

template <int FMT>
constexpr float kQMax = FMT == kInt8 ? 127.f : 448.f;

constexpr int kPass = 4 * kWave;  // channels a wave covers per pass
constexpr int kWavesPerBlock = kBlock / kWave;

inline int64_t packed_stride(int64_t F) { return (F + 4 + 15) / 16 * 16; }

inline int parse_fmt(const std::string& fmt) {
  TORCH_CHECK(fmt == "int8" || fmt == "fp8",
              "quantised format must be 'int8' or 'fp8', got '", fmt, "'");
  return fmt == "int8" ? kInt8 : kFp8;
}

typedef float float2v __attribute__((ext_vector_type(2)));

// same in all lanes, but the compiler cannot see it through threadIdx
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi =
      __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// xor butterfly: every lane ends with the wave's maximum
__device__ __forceinline__ float wave_max(float v, int lane) {
#pragma unroll
  for (int mask = 1; mask < kWave; mask <<= 1)
    v = fmaxf(v, lane_xor(v, lane, mask));
  return v;
}

template <typename T>
__device__ __forceinline__ float bits16_to_f32(uint32_t h) {
  if constexpr (std::is_same<T, c10::Half>::value) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
  } else {
    return __builtin_bit_cast(float, h << 16);
  }
}

// Channels c .. c + 3 (c < F) of a row of F as fp32, 0 past the row.  kQuad:
// F % 4 == 0 and the rows aligned to four elements, one 16- or 8-byte load.
template <typename T, bool kQuad>
__device__ __forceinline__ void load4(const T* __restrict__ row, int64_t c,
                                      int64_t F, float (&v)[4]) {
  if constexpr (kQuad) {
    if constexpr (std::is_same<T, float>::value) {
      const float4 w = *reinterpret_cast<const float4*>(row + c);
      v[0] = w.x;
      v[1] = w.y;
      v[2] = w.z;
      v[3] = w.w;
    } else {
      const uint2 w = *reinterpret_cast<const uint2*>(row + c);
      v[0] = bits16_to_f32<T>(w.x & 0xffffu);
      v[1] = bits16_to_f32<T>(w.x >> 16);
      v[2] = bits16_to_f32<T>(w.y & 0xffffu);
      v[3] = bits16_to_f32<T>(w.y >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = 0.f;
      if (c + k < F) {
        if constexpr (std::is_same<T, float>::value) {
          v[k] = row[c + k];
        } else {
          v[k] = bits16_to_f32<T>(
              reinterpret_cast<const uint16_t*>(row)[c + k]);
        }
      }
    }
  }
}

// four codes, channel k in byte k
template <int FMT>
__device__ __forceinline__ uint32_t encode4(const float (&v)[4], float inv) {
  constexpr float Q = kQMax<FMT>;
  float y[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float t = v[k] * inv;
    t = (t != t) ? 0.f : t;
    y[k] = fminf(fmaxf(t, -Q), Q);
  }
  if constexpr (FMT == kInt8) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w |= ((uint32_t)(int)rintf(y[k]) & 0xffu) << (8 * k);
    return w;
  } else {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w, true);
    return (uint32_t)w;
  }
}

// the exact values of four codes
template <int FMT>
__device__ __forceinline__ void decode4(uint32_t w, float (&v)[4]) {
  if constexpr (FMT == kInt8) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)(int8_t)(w >> (8 * k));
  } else {
    const float2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const float2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    v[0] = lo.x;
    v[1] = lo.y;
    v[2] = hi.x;
    v[3] = hi.y;
  }
}

template <typename in_t, int FMT, bool kQuad>
__global__ void __launch_bounds__(kBlock)
quantize_rows_kernel(const in_t* __restrict__ x, int64_t N, int64_t F,
                     int64_t S, uint8_t* __restrict__ out) {
  constexpr float Q = kQMax<FMT>;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave0 = wave_uniform(
      blockIdx.x * (int64_t)kWavesPerBlock + threadIdx.x / kWave);
  const int64_t stride = (int64_t)gridDim.x * kWavesPerBlock;
  const bool resident = F <= kPass;
  for (int64_t r = wave0; r < N; r += stride) {
    const in_t* row = x + r * F;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    float amax = 0.f;
    for (int64_t c = 4 * lane; c < F; c += kPass) {
      load4<in_t, kQuad>(row, c, F, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a = fabsf(v[k]);
        amax = fmaxf(amax, (a != a) ? 0.f : a);
      }
    }
    amax = wave_max(amax, lane);
    const bool live = amax >= 0x1p-119f && amax <= FLT_MAX;
    const float scale = live ? amax / Q : 0.f;
    const float inv = live ? Q / amax : 0.f;
    uint8_t* orow = out + r * S;
    // the words at and past F are the padding; S - 4 is the scale's
    for (int64_t c = 4 * lane; c < S - 4; c += kPass) {
      uint32_t w = 0;
      if (live && c < F) {
        if (!resident) load4<in_t, kQuad>(row, c, F, v);
        w = encode4<FMT>(v, inv);
      }
      *reinterpret_cast<uint32_t*>(orow + c) = w;
    }
    if (lane == 0) *reinterpret_cast<float*>(orow + S - 4) = scale;
  }
}

// 16 bytes of output in pieces of VS bytes, those at or past row_bytes
// dropped; byte0 is the chunk's offset in its row and a multiple of 16,
// row_bytes a multiple of VS.
template <int VS>
__device__ __forceinline__ void store_chunk(char* __restrict__ dst,
                                            const uint32_t (&w)[4],
                                            int64_t byte0,
                                            int64_t row_bytes) {
  if constexpr (VS == 16) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
  } else if constexpr (VS == 8) {
    if (byte0 < row_bytes)
      *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    if (byte0 + 8 < row_bytes)
      *reinterpret_cast<uint2*>(dst + 8) = make_uint2(w[2], w[3]);
  } else if constexpr (VS == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (byte0 + 4 * k < row_bytes)
        *reinterpret_cast<uint32_t*>(dst + 4 * k) = w[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (byte0 + 2 * k < row_bytes)
        *reinterpret_cast<uint16_t*>(dst + 2 * k) =
            (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
  }
}

template <int FMT, typename out_t, int VS>
__global__ void __launch_bounds__(kBlock)
gather_dequant_kernel(SegTable segs, int64_t F, int64_t S,
                      const int64_t* __restrict__ rows, int64_t n,
                      char* __restrict__ out) {
  constexpr int CH = 16 / (int)sizeof(out_t);  // codes per chunk
  const int64_t chunks = (F + CH - 1) / CH;
  const int64_t row_bytes = F * (int64_t)sizeof(out_t);
  const int64_t total = n * chunks;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / chunks;
    const int64_t j = idx - i * chunks;
    const char* src = seg_row(segs, rows[i], S);
    const float scale = *reinterpret_cast<const float*>(src + S - 4);
    // a tail chunk reads into the padding (or the scale), inside the row:
    // round_up(F, CH) <= S
    uint32_t w[4];
    if constexpr (CH == 8) {
      const uint2 c = reinterpret_cast<const uint2*>(src)[j];
      float lo[4], hi[4];
      decode4<FMT>(c.x, lo);
      decode4<FMT>(c.y, hi);
      w[0] = bf16_rne(lo[0] * scale) | (bf16_rne(lo[1] * scale) << 16);
      w[1] = bf16_rne(lo[2] * scale) | (bf16_rne(lo[3] * scale) << 16);
      w[2] = bf16_rne(hi[0] * scale) | (bf16_rne(hi[1] * scale) << 16);
      w[3] = bf16_rne(hi[2] * scale) | (bf16_rne(hi[3] * scale) << 16);
    } else {
      float v[4];
      decode4<FMT>(reinterpret_cast<const uint32_t*>(src)[j], v);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        w[k] = __builtin_bit_cast(uint32_t, v[k] * scale);
    }
    store_chunk<VS>(out + i * row_bytes + j * 16, w, j * 16, row_bytes);
  }
}

template <typename in_t, int FMT>
void launch_quantize(const torch::Tensor& x, torch::Tensor& out) {
  const int64_t N = x.size(0), F = x.size(1), S = out.size(1);
  const in_t* xp = reinterpret_cast<const in_t*>(x.data_ptr());
  const bool quad = F % 4 == 0 &&
                    reinterpret_cast<uintptr_t>(xp) % (4 * sizeof(in_t)) == 0;
  const int blocks = grid_for(N, kWavesPerBlock);
  auto stream = current_stream();
  uint8_t* op = out.data_ptr<uint8_t>();
  if (quad)
    hipLaunchKernelGGL((quantize_rows_kernel<in_t, FMT, true>), dim3(blocks),
                       dim3(kBlock), 0, stream, xp, N, F, S, op);
  else
    hipLaunchKernelGGL((quantize_rows_kernel<in_t, FMT, false>), dim3(blocks),
                       dim3(kBlock), 0, stream, xp, N, F, S, op);
}

template <int FMT, typename out_t>
void launch_gather(const SegTable& t, int64_t F, int64_t S,
                   const int64_t* rows, int64_t n, char* out) {
  constexpr int CH = 16 / (int)sizeof(out_t);
  const int64_t row_bytes = F * (int64_t)sizeof(out_t);
  const int blocks = grid_for(n * ((F + CH - 1) / CH));
  auto stream = current_stream();
#define GLT_LAUNCH_DEQUANT(VS)                                            \
  hipLaunchKernelGGL((gather_dequant_kernel<FMT, out_t, VS>),             \
                     dim3(blocks), dim3(kBlock), 0, stream, t, F, S, rows, \
                     n, out)
  if (row_bytes % 16 == 0)
    GLT_LAUNCH_DEQUANT(16);
  else if (row_bytes % 8 == 0)
    GLT_LAUNCH_DEQUANT(8);
  else if (row_bytes % 4 == 0)
    GLT_LAUNCH_DEQUANT(4);
  else if constexpr (sizeof(out_t) == 2)
    GLT_LAUNCH_DEQUANT(2);
#undef GLT_LAUNCH_DEQUANT
}

}  // namespace

torch::Tensor hip_quantize_rows(const torch::Tensor& x,
                                const std::string& fmt) {
  const int f = parse_fmt(fmt);
  TORCH_CHECK(x.is_cuda(), "quantize_rows takes a device tensor");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "quantize_rows takes a contiguous 2-D tensor");
  const auto dt = x.scalar_type();
  TORCH_CHECK(dt == torch::kFloat32 || dt == torch::kBFloat16 ||
                  dt == torch::kFloat16,
              "quantize_rows takes fp32, bf16 or fp16");
  TORCH_CHECK(x.size(1) >= 1, "quantize_rows needs at least one column");
  auto out = torch::empty(
      {x.size(0), packed_stride(x.size(1))},
      torch::TensorOptions().dtype(torch::kUInt8).device(x.device()));
  if (x.size(0) == 0) return out;
#define GLT_QUANT_DTYPE(T)            \
  if (f == kInt8)                     \
    launch_quantize<T, kInt8>(x, out); \
  else                                \
    launch_quantize<T, kFp8>(x, out)
  if (dt == torch::kFloat32) {
    GLT_QUANT_DTYPE(float);
  } else if (dt == torch::kBFloat16) {
    GLT_QUANT_DTYPE(c10::BFloat16);
  } else {
    GLT_QUANT_DTYPE(c10::Half);
  }
#undef GLT_QUANT_DTYPE
  return out;
}

class QuantFeatureStore {
 public:
  QuantFeatureStore(int64_t device_index, int64_t dim, const std::string& fmt)
      : device_(torch::kCUDA, (int8_t)device_index),
        dim_(dim),
        stride_(packed_stride(dim)),
        fmt_(parse_fmt(fmt)) {
    TORCH_CHECK(dim >= 1, "feature dim must be positive");
  }

  void append(const torch::Tensor& seg) {
    TORCH_CHECK(seg.is_cuda(),
                "segments must be device tensors or host-mapped views");
    TORCH_CHECK(seg.scalar_type() == torch::kUInt8,
                "packed segments are uint8");
    TORCH_CHECK(seg.dim() == 2, "segment must be 2-D [rows, stride]");
    TORCH_CHECK(seg.is_contiguous(), "segment must be contiguous");
    TORCH_CHECK(seg.size(1) == stride_, "packed rows of dim ", dim_, " are ",
                stride_, " bytes wide, got ", seg.size(1));
    TORCH_CHECK((int)segs_.size() < kMaxSegs, "too many segments");
    segs_.push_back(seg);
    rows_ += seg.size(0);
  }

  torch::Tensor gather(const torch::Tensor& rows, torch::ScalarType out_dtype) {
    TORCH_CHECK(!segs_.empty(), "empty feature store");
    TORCH_CHECK(out_dtype == torch::kFloat32 || out_dtype == torch::kBFloat16,
                "dequantised rows are fp32 or bf16");
    TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == torch::kInt64,
                "row indices must be int64 on the device");
    TORCH_CHECK(rows.dim() == 1 && rows.is_contiguous(),
                "row indices must be a contiguous 1-D tensor");
    const int64_t n = rows.size(0);
    auto out = torch::empty(
        {n, dim_}, torch::TensorOptions().dtype(out_dtype).device(device_));
    if (n == 0) return out;
    const SegTable t = make_seg_table(segs_);
    const int64_t* rp = rows.data_ptr<int64_t>();
    char* op = reinterpret_cast<char*>(out.data_ptr());
    const bool bf16 = out_dtype == torch::kBFloat16;
    if (fmt_ == kInt8) {
      if (bf16)
        launch_gather<kInt8, c10::BFloat16>(t, dim_, stride_, rp, n, op);
      else
        launch_gather<kInt8, float>(t, dim_, stride_, rp, n, op);
    } else {
      if (bf16)
        launch_gather<kFp8, c10::BFloat16>(t, dim_, stride_, rp, n, op);
      else
        launch_gather<kFp8, float>(t, dim_, stride_, rp, n, op);
    }
    return out;
  }

  int64_t rows() const { return rows_; }
  int64_t dim() const { return dim_; }

 private:
  torch::Device device_;
  std::vector<torch::Tensor> segs_;
  int64_t rows_ = 0;
  int64_t dim_;
  int64_t stride_;
  int fmt_;
};

std::shared_ptr<QuantFeatureStore> qfs_create(int64_t device_index,
                                              int64_t dim,
                                              const std::string& fmt) {
  return std::make_shared<QuantFeatureStore>(device_index, dim, fmt);
}
void qfs_append(QuantFeatureStore* s, const torch::Tensor& seg) {
  s->append(seg);
}
torch::Tensor qfs_gather(QuantFeatureStore* s, const torch::Tensor& rows,
                         torch::ScalarType out_dtype) {
  return s->gather(rows, out_dtype);
}
int64_t qfs_rows(QuantFeatureStore* s) { return s->rows(); }
int64_t qfs_dim(QuantFeatureStore* s) { return s->dim(); }

}  // namespace glt

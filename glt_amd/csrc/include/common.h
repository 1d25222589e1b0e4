/* glt_amd common definitions.
 *
 * MI355X-native GNN sampling engine — shared CPU/HIP declarations.
 * Re-designed from scratch; behavioral parity targets are cited against
 * the reference (alibaba/graphlearn-for-pytorch) as file:line where relevant.
 */
#pragma once

#include <torch/extension.h>

#include <cstdint>
#include <atomic>
#include <random>

namespace glt {

// ---------------------------------------------------------------------------
// Deterministic seeding.
//
// A single process-wide base seed (set from python via manual_seed) combined
// with a monotonically increasing call counter, split per row/lane with
// splitmix64.  This gives reproducible sampling runs when the user seeds,
// while every call still draws fresh randomness.
// Parity target: RandomSeedManager (reference include/common.h, bound at
// python/py_export_glt.cc:84-87).
// ---------------------------------------------------------------------------
class SeedManager {
 public:
  static SeedManager& instance() {
    static SeedManager inst;
    return inst;
  }
  void set_seed(uint64_t s) {
    base_.store(s, std::memory_order_relaxed);
    counter_.store(0, std::memory_order_relaxed);
    seeded_.store(true, std::memory_order_relaxed);
  }
  bool seeded() const { return seeded_.load(std::memory_order_relaxed); }
  // One fresh 64-bit stream id per sampling call.
  uint64_t next_call_seed() {
    uint64_t c = counter_.fetch_add(1, std::memory_order_relaxed);
    uint64_t b = seeded_.load(std::memory_order_relaxed)
                     ? base_.load(std::memory_order_relaxed)
                     : std::random_device{}();
    return b * 0x9E3779B97F4A7C15ull + c + 1;
  }

 private:
  std::atomic<uint64_t> base_{0x243F6A8885A308D3ull};
  std::atomic<uint64_t> counter_{0};
  std::atomic<bool> seeded_{false};
};

// splitmix64: cheap, high-quality 64-bit mixer; used to derive per-row RNG
// streams on both CPU and GPU so results are device-independent in structure
// (not bitwise — different generators).
inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Fast 64-bit PCG-ish generator for CPU sampling paths (cheaper than mt19937
// to construct per row).
struct Rng64 {
  uint64_t state;
  explicit Rng64(uint64_t seed) : state(splitmix64(seed)) {}
  inline uint64_t next() {
    // xorshift64*
    uint64_t x = state;
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    state = x;
    return x * 0x2545F4914F6CDD1Dull;
  }
  // uniform integer in [0, n) without modulo bias (Lemire).
  inline uint64_t uniform(uint64_t n) {
    __uint128_t m = (__uint128_t)next() * (__uint128_t)n;
    return (uint64_t)(m >> 64);
  }
  inline float uniform_float() {  // [0, 1)
    return (next() >> 40) * (1.0f / 16777216.0f);
  }
};

// Host twins of the device Feistel permutation (hip/hip_common.h
// feistel_perm / feistel_perm_inv): bit-identical, so the round trip can be
// tested without a GPU.
inline uint32_t feistel_round_host(uint32_t x, uint32_t key) {
  x = (x ^ key) * 0x9E3779B9u;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  return x;
}

inline uint32_t feistel_round_key(uint32_t k0, uint32_t k1, int round) {
  return k0 + round * 0x7F4A7C15u + (round & 1 ? k1 : 0);
}

inline uint32_t feistel_half_bits(uint64_t n) {
  uint32_t total_bits =
      64 - __builtin_clzll((unsigned long long)(n - 1) | 1ull);
  uint32_t hb = (total_bits + 1) >> 1;
  return hb < 1 ? 1 : hb;
}

inline uint64_t feistel_perm_host(uint64_t key64, uint64_t j, uint64_t n) {
  const uint32_t hb = feistel_half_bits(n);
  const uint32_t hmask = (1u << hb) - 1u;
  const uint32_t k0 = (uint32_t)key64, k1 = (uint32_t)(key64 >> 32);
  uint64_t x = j;
  do {
    uint32_t l = (uint32_t)(x >> hb) & hmask;
    uint32_t r = (uint32_t)x & hmask;
    for (int round = 0; round < 6; ++round) {
      uint32_t nl = r;
      r = l ^ (feistel_round_host(r, feistel_round_key(k0, k1, round)) &
               hmask);
      l = nl;
    }
    x = ((uint64_t)l << hb) | r;
  } while (x >= n);
  return x;
}

// Inverse: the six rounds backwards, (l, r) <- (r ^ F(l), l), cycle-walking
// with the inverse until the result is < n.
inline uint64_t feistel_perm_inv_host(uint64_t key64, uint64_t y,
                                      uint64_t n) {
  const uint32_t hb = feistel_half_bits(n);
  const uint32_t hmask = (1u << hb) - 1u;
  const uint32_t k0 = (uint32_t)key64, k1 = (uint32_t)(key64 >> 32);
  uint64_t x = y;
  do {
    uint32_t l = (uint32_t)(x >> hb) & hmask;
    uint32_t r = (uint32_t)x & hmask;
    for (int round = 5; round >= 0; --round) {
      uint32_t nr = l;
      l = r ^ (feistel_round_host(l, feistel_round_key(k0, k1, round)) &
               hmask);
      r = nr;
    }
    x = ((uint64_t)l << hb) | r;
  } while (x >= n);
  return x;
}

inline void check_int64_1d(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 1, name, " must be 1-D");
  TORCH_CHECK(t.scalar_type() == torch::kInt64, name, " must be int64");
}

// Argument checks shared by cpu_/hip_sample_neighbors_temporal; every one
// raises before any launch.
inline void check_temporal_args(
    const torch::Tensor& indptr, const torch::Tensor& indices,
    const c10::optional<torch::Tensor>& edge_ids, const torch::Tensor& seeds,
    const torch::Tensor& seed_time,
    const c10::optional<torch::Tensor>& edge_time,
    const c10::optional<torch::Tensor>& node_time, bool with_edge) {
  TORCH_CHECK(edge_time.has_value() != node_time.has_value(),
              "sample_neighbors_temporal: exactly one of edge_time / "
              "node_time must be given");
  TORCH_CHECK(!with_edge || edge_ids.has_value(),
              "with_edge requires edge_ids");
  auto chk = [&](const torch::Tensor& t, const char* name) {
    check_int64_1d(t, name);
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(t.device() == indptr.device(), name,
                " must be on the same device as indptr");
  };
  chk(indptr, "indptr");
  TORCH_CHECK(indptr.numel() >= 1, "indptr must not be empty");
  chk(indices, "indices");
  chk(seeds, "seeds");
  chk(seed_time, "seed_time");
  if (edge_ids.has_value()) {
    chk(*edge_ids, "edge_ids");
    TORCH_CHECK(edge_ids->numel() == indices.numel(),
                "edge_ids must have one entry per edge");
  }
  TORCH_CHECK(seed_time.numel() == seeds.numel(),
              "seed_time must have one entry per seed");
  if (edge_time.has_value()) {
    chk(*edge_time, "edge_time");
    TORCH_CHECK(edge_time->numel() == indices.numel(),
                "edge_time must have one entry per edge");
  } else {
    chk(*node_time, "node_time");
    TORCH_CHECK(node_time->numel() >= indptr.numel() - 1,
                "node_time must cover every row");
  }
}

}  // namespace glt

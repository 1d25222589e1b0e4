/* Deferred-sync multi-hop sampling (gfx950).
 *
 * The classic pipeline syncs the host once per hop for the sampled-edge
 * total and once per hop for the new-node count (reference does the same,
 * random_sampler.cu:296-300).  Here every intermediate count lives in
 * device memory and every kernel guards its work on those device scalars,
 * so an L-hop batch runs with ZERO host round trips; the python layer
 * reads one packed [2L] counts tensor at the end (single sync per batch).
 *
 * Buffers are capacity-sized (no-dedup worst case, a pure function of
 * batch x fan-out); tails beyond the device counts are never read.
 */
#include "hip_common.h"
#include "../include/common.h"
#include "../include/hip_ops.h"

namespace glt {

namespace {

constexpr uint64_t kEmpty = ~0ull;
constexpr unsigned long long kNoIndex = 0x7FFFFFFFFFFFFFFFull;

// One table slot: everything a probe needs lies in one 32-byte sector, so a
// probe touches one cache line and the CAS on the key and the atomicMin on
// the first index of one insert go to the same line.
struct alignas(32) DSlot {
  unsigned long long key;        // kEmpty until claimed
  unsigned long long first_idx;  // least element index that inserted the key
  int64_t local_id;              // -1 until d_assign_kernel numbers the key
  int64_t pad;
};
static_assert(sizeof(DSlot) == 32, "one slot is one 32-byte sector");

struct DTableView {
  DSlot* slots;
  uint64_t mask;
};

__device__ __forceinline__ uint64_t d_probe(uint64_t key, uint64_t mask) {
  return d_splitmix64(key) & mask;
}

// Sum of the first m entries of stats (m <= L + 1): the number of nodes
// numbered before a hop.  Every kernel that needs the running count adds the
// few entries itself; there is no separate counter to bump.
__device__ __forceinline__ int64_t d_nodes_before(
    const int64_t* __restrict__ stats, int m) {
  int64_t s = 0;
  for (int i = 0; i < m; ++i) s += stats[i];
  return s;
}

// The whole per-batch reset in one launch: empties every slot and stores the
// seed count the seed pass guards on.
__global__ void d_reset_kernel(DTableView t, int64_t* __restrict__ seed_n,
                               int64_t bs) {
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    DSlot s;
    s.key = kEmpty;
    s.first_idx = kNoIndex;
    s.local_id = -1;
    s.pad = 0;
    t.slots[i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *seed_n = bs;
}

__global__ void d_fill_counts_kernel(const int64_t* __restrict__ indptr,
                                     int64_t num_rows,
                                     const int64_t* __restrict__ seeds,
                                     const int64_t* __restrict__ n_dev,
                                     int64_t cap, int64_t k,
                                     int64_t* __restrict__ counts) {
  const int64_t n = *n_dev;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = 0;
    if (i < n) {
      const int64_t v = seeds[i];
      const int64_t deg =
          (v >= 0 && v < num_rows) ? indptr[v + 1] - indptr[v] : 0;
      c = deg < k ? deg : k;
    }
    counts[i] = c;
  }
}

// Samples hop `hop` and writes its rows as well: the frontier is the
// previous hop's new nodes in rank order (the unique seeds for hop 0), so
// frontier element r has local id (nodes numbered before the frontier) + r
// and no table lookup is needed.  One thread also stores the hop's edge
// total to stats_total.
template <bool WITH_EID>
__global__ void d_sample_gather_kernel(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
    const int64_t* __restrict__ eids, int64_t num_rows,
    const int64_t* __restrict__ seeds, const int64_t* __restrict__ n_dev,
    int64_t cap, int64_t k, const int64_t* __restrict__ offsets,
    uint64_t call_seed, const int64_t* __restrict__ stats, int hop,
    int64_t* __restrict__ stats_total, int64_t* __restrict__ out_nbrs,
    int64_t* __restrict__ out_eids, int64_t* __restrict__ out_rows) {
  const int64_t n = *n_dev;
  const int64_t total = offsets[n];
  const int64_t frontier_base = d_nodes_before(stats, hop);
  if (blockIdx.x == 0 && threadIdx.x == 0) *stats_total = total;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = row_of(offsets, n, e);
    const int64_t j = e - offsets[r];
    const int64_t v = seeds[r];
    const int64_t base = indptr[v];
    const int64_t deg = indptr[v + 1] - base;
    int64_t pos;
    if (deg <= k) {
      pos = j;
    } else {
      pos = (int64_t)feistel_perm(d_splitmix64(call_seed + (uint64_t)r),
                                  (uint64_t)j, (uint64_t)deg);
    }
    out_nbrs[e] = indices[base + pos];
    if (WITH_EID) out_eids[e] = eids[base + pos];
    out_rows[e] = frontier_base + r;
  }
}

// The one probe per element: claims or finds the key's slot, lowers the
// slot's first index to i and records the slot for the flag, assign and
// relabel passes, which then neither hash nor walk.
__global__ void d_insert_kernel(DTableView t,
                                const int64_t* __restrict__ ids,
                                const int64_t* __restrict__ n_dev,
                                int64_t cap, int32_t* __restrict__ slot_of) {
  const int64_t n = *n_dev;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= n) continue;
    const uint64_t key = (uint64_t)ids[i];
    uint64_t slot = d_probe(key, t.mask);
    for (;;) {
      const uint64_t prev =
          atomicCAS(&t.slots[slot].key, (unsigned long long)kEmpty,
                    (unsigned long long)key);
      if (prev == kEmpty || prev == key) {
        atomicMin(&t.slots[slot].first_idx, (unsigned long long)i);
        break;
      }
      slot = (slot + 1) & t.mask;
    }
    slot_of[i] = (int32_t)slot;
  }
}

__global__ void d_flag_kernel(DTableView t,
                              const int32_t* __restrict__ slot_of,
                              const int64_t* __restrict__ n_dev,
                              int64_t cap, int64_t* __restrict__ flags) {
  const int64_t n = *n_dev;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t f = 0;
    if (i < n) {
      const DSlot& s = t.slots[slot_of[i]];
      f = (s.local_id < 0 && s.first_idx == (unsigned long long)i) ? 1 : 0;
    }
    flags[i] = f;
  }
}

// Numbers the flagged (first-occurrence, not yet numbered) elements from
// the sum of the first n_before entries of stats and stores the count of
// new nodes to n_new_out, an entry of stats past those.
__global__ void d_assign_kernel(DTableView t,
                                const int64_t* __restrict__ ids,
                                const int32_t* __restrict__ slot_of,
                                const int64_t* __restrict__ n_dev,
                                int64_t cap,
                                const int64_t* __restrict__ ranks,
                                const int64_t* __restrict__ flags,
                                const int64_t* __restrict__ stats,
                                int n_before,
                                int64_t* __restrict__ unique_out,
                                int64_t* __restrict__ n_new_out) {
  const int64_t n = *n_dev;
  const int64_t base = d_nodes_before(stats, n_before);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n && flags[i]) {
      t.slots[slot_of[i]].local_id = base + ranks[i] - 1;
      unique_out[ranks[i] - 1] = ids[i];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *n_new_out = n > 0 ? ranks[n - 1] : 0;
  }
}

// out[i] = local id of the key element i inserted.  Every element below the
// device count went through d_insert_kernel and its key was numbered by
// this or an earlier d_assign_kernel, so each gets a local id >= 0.  The
// one exception the contract leaves is the id -1: it equals the empty mark,
// claims no slot of its own, and reads back whatever its recorded slot
// holds, -1 where that slot was never numbered.
__global__ void d_relabel_kernel(DTableView t,
                                 const int32_t* __restrict__ slot_of,
                                 const int64_t* __restrict__ total_dev,
                                 int64_t cap, int64_t* __restrict__ out) {
  const int64_t n = *total_dev;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= n) continue;
    out[i] = t.slots[slot_of[i]].local_id;
  }
}

int64_t d_next_pow2(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

}  // namespace

// ---------------------------------------------------------------------------
// DeferredSampler: holds all capacity buffers + the hash table and runs an
// L-hop batch without host syncs.  One instance per (device, fanout) — the
// python layer pools them like inducers.
// ---------------------------------------------------------------------------
class DeferredSampler {
 public:
  DeferredSampler(std::vector<int64_t> fanout, int64_t batch_cap,
                  torch::Device device, bool with_eid)
      : fanout_(std::move(fanout)), with_eid_(with_eid), device_(device) {
    TORCH_CHECK(!fanout_.empty(), "deferred sampler needs >=1 hop");
    for (auto k : fanout_)
      TORCH_CHECK(k > 0, "deferred sampler needs positive fan-outs");
    auto opts = torch::TensorOptions().dtype(torch::kInt64).device(device);
    int64_t cap = batch_cap;
    node_cap_ = {cap};
    for (auto k : fanout_) {
      cap *= k;
      node_cap_.push_back(cap);
    }
    total_node_cap_ = 0;
    for (auto c : node_cap_) total_node_cap_ += c;
    // hash table sized for every node of the batch
    table_cap_ = d_next_pow2(total_node_cap_ * 2);
    TORCH_CHECK(table_cap_ <= ((int64_t)1 << 31),
                "deferred: table too large for 32-bit slot records");
    table_ = torch::empty({table_cap_ * (int64_t)(sizeof(DSlot) / 8)}, opts);
    auto slot_opts = opts.dtype(torch::kInt32);
    for (size_t h = 0; h < fanout_.size(); ++h) {
      const int64_t rc = node_cap_[h];
      const int64_t ec = node_cap_[h + 1];
      counts_.push_back(torch::empty({rc}, opts));
      offsets_.push_back(torch::zeros({rc + 1}, opts));
      nbrs_.push_back(torch::empty({ec}, opts));
      eids_.push_back(with_eid ? torch::empty({ec}, opts)
                               : torch::Tensor());
      rows_.push_back(torch::empty({ec}, opts));
      cols_.push_back(torch::empty({ec}, opts));
      uniq_.push_back(torch::empty({ec}, opts));
      flags_.push_back(torch::empty({ec}, opts));
      slot_.push_back(torch::empty({ec}, slot_opts));
    }
    seed_uniq_ = torch::empty({batch_cap}, opts);
    seed_flags_ = torch::empty({batch_cap}, opts);
    seed_slot_ = torch::empty({batch_cap}, slot_opts);
    seed_n_ = torch::zeros({1}, opts);
    stats_ = torch::zeros({(int64_t)(2 * fanout_.size() + 1)}, opts);
  }

  // Runs the whole multi-hop batch; returns
  // (node parts, rows list, cols list, eids list, stats) where stats
  // = [n_seed_uniq, n_new_1.., total_e_1..] lives on DEVICE until the
  // caller's single .cpu() read.
  std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>,
             std::vector<torch::Tensor>, std::vector<torch::Tensor>,
             torch::Tensor>
  run(const torch::Tensor& indptr, const torch::Tensor& indices,
      const c10::optional<torch::Tensor>& edge_ids,
      const torch::Tensor& seeds_in) {
    auto stream = current_stream();
    TORCH_CHECK(seeds_in.scalar_type() == torch::kInt64,
                "deferred: seeds must be int64");
    TORCH_CHECK(seeds_in.device() == device_,
                "deferred: seeds on wrong device");
    TORCH_CHECK(!with_eid_ || edge_ids.has_value(),
                "deferred: with_eid sampler needs edge_ids");
    auto seeds = seeds_in.contiguous();
    const int64_t num_rows = indptr.size(0) - 1;
    const int64_t bs = seeds.size(0);
    TORCH_CHECK(bs <= node_cap_[0], "batch exceeds deferred capacity");
    DTableView t = view();
    int64_t* stats = stats_.data_ptr<int64_t>();
    // empty table + seed count, one launch
    hipLaunchKernelGGL(d_reset_kernel, dim3(grid_for(table_cap_)),
                       dim3(kBlock), 0, stream, t,
                       seed_n_.data_ptr<int64_t>(), bs);
    // dedup seeds
    hipLaunchKernelGGL(d_insert_kernel, dim3(grid_for(bs)), dim3(kBlock), 0,
                       stream, t, seeds.data_ptr<int64_t>(),
                       seed_n_.data_ptr<int64_t>(), bs,
                       seed_slot_.data_ptr<int32_t>());
    hipLaunchKernelGGL(d_flag_kernel, dim3(grid_for(bs)), dim3(kBlock), 0,
                       stream, t, seed_slot_.data_ptr<int32_t>(),
                       seed_n_.data_ptr<int64_t>(), bs,
                       seed_flags_.data_ptr<int64_t>());
    auto seed_ranks = torch::cumsum(seed_flags_.narrow(0, 0, bs), 0);
    hipLaunchKernelGGL(d_assign_kernel, dim3(grid_for(bs)), dim3(kBlock), 0,
                       stream, t, seeds.data_ptr<int64_t>(),
                       seed_slot_.data_ptr<int32_t>(),
                       seed_n_.data_ptr<int64_t>(), bs,
                       seed_ranks.data_ptr<int64_t>(),
                       seed_flags_.data_ptr<int64_t>(), stats, 0,
                       seed_uniq_.data_ptr<int64_t>(),
                       stats);  // stats[0] = n_seed

    const int64_t L = (int64_t)fanout_.size();
    const int64_t* eid_ptr =
        edge_ids.has_value() ? edge_ids->data_ptr<int64_t>() : nullptr;
    torch::Tensor frontier = seed_uniq_;
    for (int64_t h = 0; h < L; ++h) {
      const int64_t rc = node_cap_[h];
      const int64_t ec = node_cap_[h + 1];
      const int64_t k = fanout_[h];
      const int64_t* frontier_n = stats + h;
      const uint64_t cs = SeedManager::instance().next_call_seed();
      hipLaunchKernelGGL(d_fill_counts_kernel, dim3(grid_for(rc)),
                         dim3(kBlock), 0, stream,
                         indptr.data_ptr<int64_t>(), num_rows,
                         frontier.data_ptr<int64_t>(), frontier_n, rc, k,
                         counts_[h].data_ptr<int64_t>());
      {
        auto v = offsets_[h].narrow(0, 1, rc);
        torch::cumsum_out(v, counts_[h], 0);
      }
      // neighbours, edge ids and rows of hop h; the hop's edge total goes
      // to stats[L + 1 + h] from the same launch
      const bool eid = with_eid_ && eid_ptr;
      hipLaunchKernelGGL(
          eid ? d_sample_gather_kernel<true> : d_sample_gather_kernel<false>,
          dim3(grid_for(ec)), dim3(kBlock), 0, stream,
          indptr.data_ptr<int64_t>(), indices.data_ptr<int64_t>(), eid_ptr,
          num_rows, frontier.data_ptr<int64_t>(), frontier_n, rc, k,
          offsets_[h].data_ptr<int64_t>(), cs, stats, (int)h,
          stats + L + 1 + h, nbrs_[h].data_ptr<int64_t>(),
          eid ? eids_[h].data_ptr<int64_t>() : nullptr,
          rows_[h].data_ptr<int64_t>());
      // insert neighbors, assign fresh local ids
      const int64_t* total_dev = offsets_[h].data_ptr<int64_t>() + rc;
      hipLaunchKernelGGL(d_insert_kernel, dim3(grid_for(ec)), dim3(kBlock),
                         0, stream, t, nbrs_[h].data_ptr<int64_t>(),
                         total_dev, ec, slot_[h].data_ptr<int32_t>());
      hipLaunchKernelGGL(d_flag_kernel, dim3(grid_for(ec)), dim3(kBlock), 0,
                         stream, t, slot_[h].data_ptr<int32_t>(), total_dev,
                         ec, flags_[h].data_ptr<int64_t>());
      auto ranks = torch::cumsum(flags_[h], 0);
      hipLaunchKernelGGL(d_assign_kernel, dim3(grid_for(ec)), dim3(kBlock),
                         0, stream, t, nbrs_[h].data_ptr<int64_t>(),
                         slot_[h].data_ptr<int32_t>(), total_dev, ec,
                         ranks.data_ptr<int64_t>(),
                         flags_[h].data_ptr<int64_t>(), stats, (int)h + 1,
                         uniq_[h].data_ptr<int64_t>(), stats + 1 + h);
      // relabel cols
      hipLaunchKernelGGL(d_relabel_kernel, dim3(grid_for(ec)), dim3(kBlock),
                         0, stream, t, slot_[h].data_ptr<int32_t>(),
                         total_dev, ec, cols_[h].data_ptr<int64_t>());
      frontier = uniq_[h];
    }
    std::vector<torch::Tensor> eids_out;
    if (with_eid_)
      for (auto& e : eids_) eids_out.push_back(e);
    // capacity-sized node parts: python slices each with stats after its
    // single end-of-batch sync
    std::vector<torch::Tensor> node_parts = {seed_uniq_};
    for (auto& u : uniq_) node_parts.push_back(u);
    return {node_parts, rows_, cols_, eids_out, stats_};
  }

 private:
  DTableView view() {
    DTableView t;
    t.slots = reinterpret_cast<DSlot*>(table_.data_ptr());
    t.mask = (uint64_t)table_cap_ - 1;
    return t;
  }

  std::vector<int64_t> fanout_, node_cap_;
  bool with_eid_;
  torch::Device device_;
  int64_t table_cap_ = 0, total_node_cap_ = 0;
  torch::Tensor table_;
  torch::Tensor seed_uniq_, seed_flags_, seed_slot_, seed_n_, stats_;
  std::vector<torch::Tensor> counts_, offsets_, nbrs_, eids_, rows_, cols_,
      uniq_, flags_, slot_;
};

std::shared_ptr<DeferredSampler> deferred_sampler_create(
    std::vector<int64_t> fanout, int64_t batch_cap, int64_t device,
    bool with_eid) {
  return std::make_shared<DeferredSampler>(
      std::move(fanout), batch_cap, torch::Device(torch::kCUDA, device),
      with_eid);
}

std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>,
           std::vector<torch::Tensor>, std::vector<torch::Tensor>,
           torch::Tensor>
deferred_sampler_run(DeferredSampler* s, const torch::Tensor& indptr,
                     const torch::Tensor& indices,
                     const c10::optional<torch::Tensor>& edge_ids,
                     const torch::Tensor& seeds) {
  return s->run(indptr, indices, edge_ids, seeds);
}

}  // namespace glt

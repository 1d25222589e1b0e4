/* Host-callable declarations for the HIP (gfx950) kernels.
 *
 * bindings.cpp is compiled by the host compiler, so everything HIP-side is
 * exposed as plain functions + opaque handles here; implementations live in
 * csrc/hip/*.hip.
 */
#pragma once

#include <torch/extension.h>

#include <memory>
#include <string>
#include <vector>

namespace glt {

// --- samplers (hip_sampler.hip) -------------------------------------------
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>>
hip_sample_neighbors(const torch::Tensor& indptr, const torch::Tensor& indices,
                     const c10::optional<torch::Tensor>& edge_ids,
                     const c10::optional<torch::Tensor>& edge_weights,
                     const torch::Tensor& seeds, int64_t k, bool with_edge,
                     bool weighted, bool replace = true);
// Staged sampling: stage 1 (counts+offsets, no host sync) lets callers
// batch the totals sync across edge types; stage 2 gathers.
std::tuple<torch::Tensor, torch::Tensor> hip_sample_neighbors_offsets(
    const torch::Tensor& indptr, const torch::Tensor& seeds, int64_t k);
std::tuple<torch::Tensor, c10::optional<torch::Tensor>>
hip_sample_neighbors_gather(const torch::Tensor& indptr,
                            const torch::Tensor& indices,
                            const c10::optional<torch::Tensor>& edge_ids,
                            const c10::optional<torch::Tensor>& edge_weights,
                            const torch::Tensor& seeds, int64_t k,
                            const torch::Tensor& offsets, int64_t total,
                            bool with_edge, bool weighted, bool replace);
// Temporal one-hop sample: only edges with time <= seed_time[i] are
// candidates; exactly one of edge_time [E] / node_time [N] is given.
std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>>
hip_sample_neighbors_temporal(const torch::Tensor& indptr,
                              const torch::Tensor& indices,
                              const c10::optional<torch::Tensor>& edge_ids,
                              const torch::Tensor& seeds,
                              const torch::Tensor& seed_time,
                              const c10::optional<torch::Tensor>& edge_time,
                              const c10::optional<torch::Tensor>& node_time,
                              int64_t k, bool with_edge, bool last);
torch::Tensor hip_lookup_degree(const torch::Tensor& indptr,
                                const torch::Tensor& nodes);
torch::Tensor hip_sample_negative(const torch::Tensor& indptr,
                                  const torch::Tensor& indices,
                                  int64_t num_cols, int64_t req_num,
                                  int64_t trials, bool padding);
torch::Tensor hip_random_walk(const torch::Tensor& indptr,
                              const torch::Tensor& indices,
                              const torch::Tensor& seeds, int64_t walk_len);
torch::Tensor hip_cal_nbr_prob(const torch::Tensor& indptr,
                               const torch::Tensor& indices,
                               const torch::Tensor& last_prob,
                               const torch::Tensor& nodes, int64_t k);

// --- inducer / subgraph / stitch (hip_inducer.hip) -------------------------
class HIPInducer;
std::shared_ptr<HIPInducer> hip_inducer_create(int64_t reserve);
torch::Tensor hip_inducer_init_node(HIPInducer* ind, const torch::Tensor& s);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
hip_inducer_induce_next(HIPInducer* ind, const torch::Tensor& srcs,
                        const torch::Tensor& nbrs,
                        const torch::Tensor& nbrs_num);
torch::Tensor hip_inducer_lookup(HIPInducer* ind, const torch::Tensor& ids);
torch::Tensor hip_inducer_insert(HIPInducer* ind, const torch::Tensor& ids);
// Staged inserts (one totals sync per hop; see HIPInducer comments).
void hip_inducer_reserve(HIPInducer* ind, int64_t total);
std::tuple<torch::Tensor, torch::Tensor> hip_inducer_insert_begin(
    HIPInducer* ind, const torch::Tensor& ids, int64_t idx_base);
torch::Tensor hip_inducer_insert_commit(HIPInducer* ind,
                                        const torch::Tensor& ids,
                                        const torch::Tensor& flags,
                                        const torch::Tensor& ranks,
                                        int64_t n_new);
int64_t hip_inducer_count(HIPInducer* ind);

// --- deferred-sync multi-hop sampler (hip_deferred.hip) ---------------------
// Runs an entire L-hop batch (sample + dedup + relabel) with zero host
// round-trips; all counts stay on device until the caller's single read of
// the returned stats tensor [n_seed, n_new_1..L, total_e_1..L].
class DeferredSampler;
std::shared_ptr<DeferredSampler> deferred_sampler_create(
    std::vector<int64_t> fanout, int64_t batch_cap, int64_t device,
    bool with_eid);
std::tuple<std::vector<torch::Tensor>, std::vector<torch::Tensor>,
           std::vector<torch::Tensor>, std::vector<torch::Tensor>,
           torch::Tensor>
deferred_sampler_run(DeferredSampler* s, const torch::Tensor& indptr,
                     const torch::Tensor& indices,
                     const c10::optional<torch::Tensor>& edge_ids,
                     const torch::Tensor& seeds);

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor,
           c10::optional<torch::Tensor>>
hip_node_subgraph(const torch::Tensor& indptr, const torch::Tensor& indices,
                  const c10::optional<torch::Tensor>& edge_ids,
                  const torch::Tensor& nodes, bool with_edge);

std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>>
hip_stitch_sample_results(int64_t ids_count,
                          const std::vector<torch::Tensor>& idx_list,
                          const std::vector<torch::Tensor>& nbrs_list,
                          const std::vector<torch::Tensor>& nbrs_num_list,
                          const std::vector<torch::Tensor>& eids_list);

// --- fused segment aggregation (hip_segment.hip) ----------------------------
torch::Tensor hip_segment_mean_fwd(const torch::Tensor& x,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   int64_t n_tgt);
torch::Tensor hip_segment_mean_bwd(const torch::Tensor& dy,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   int64_t n_src,
                                   bool order_independent = false);
// Fused [mean-agg | x-prefix] assembly (skips the dim-1 torch.cat).
torch::Tensor hip_segment_mean_cat_fwd(const torch::Tensor& x,
                                       const torch::Tensor& col,
                                       const torch::Tensor& offsets,
                                       int64_t n_tgt);
torch::Tensor hip_segment_mean_cat_bwd(const torch::Tensor& dy,
                                       const torch::Tensor& col,
                                       const torch::Tensor& offsets,
                                       int64_t n_src,
                                       bool order_independent = false);

// Atomic-free backward of the two above.  hip_segment_transpose builds the
// inverted index of col: in_edge[src_off[s] : src_off[s + 1]] lists the
// edges with col[e] == s in ascending e, as tgt[e] when tgt is given (the
// form the gather backward takes) and as e otherwise.  The gather backward
// sums per source row in fp32 and returns dx [n_src, F] in dy's dtype,
// every row written; mask ([>= n_src, F], dy's dtype) applies
// threshold_backward(dx, mask, 0) in the same pass.
std::tuple<torch::Tensor, torch::Tensor> hip_segment_transpose(
    const torch::Tensor& col, int64_t n_src,
    const c10::optional<torch::Tensor>& tgt);
torch::Tensor hip_segment_mean_bwd_gather(
    const torch::Tensor& dy, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_src, bool order_independent,
    const torch::Tensor& src_off, const torch::Tensor& in_edge,
    const c10::optional<torch::Tensor>& mask);
torch::Tensor hip_segment_mean_cat_bwd_gather(
    const torch::Tensor& dy, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_src, bool order_independent,
    const torch::Tensor& src_off, const torch::Tensor& in_edge,
    const c10::optional<torch::Tensor>& mask);

// Weighted segment sum: out[t] = a[t] * sum_e w[e] * b[col[e]] * x[col[e]]
// with optional fp32 factors (absent = 1).  bwd returns (dx fp32, dw fp32),
// each None unless requested; x is only read for dw.  coef_bound: 0-dim
// fp32 device bound on |a| |w| |b|, used in order-independent mode.
torch::Tensor hip_segment_wsum_fwd(const torch::Tensor& x,
                                   const torch::Tensor& col,
                                   const torch::Tensor& offsets,
                                   const c10::optional<torch::Tensor>& w,
                                   const c10::optional<torch::Tensor>& a,
                                   const c10::optional<torch::Tensor>& b);
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
hip_segment_wsum_bwd(const torch::Tensor& dy,
                     const c10::optional<torch::Tensor>& x,
                     const torch::Tensor& col, const torch::Tensor& offsets,
                     const c10::optional<torch::Tensor>& w,
                     const c10::optional<torch::Tensor>& a,
                     const c10::optional<torch::Tensor>& b, int64_t n_src,
                     bool need_dx, bool need_dw, bool order_independent,
                     const c10::optional<torch::Tensor>& coef_bound);

// Segment max / min: out[t, f] = extreme over the segment of x[col[e], f],
// arg[t, f] = col of the FIRST edge attaining it (strict compare, NaN
// wins; empty segment: out 0, arg -1).  cat: out is [n_tgt, 2F] with
// out[t, F:] = x[t, :].  fwd returns (out, arg int32 [n_tgt, F] or None
// without need_arg); bwd returns fp32 dx with dx[arg[t, f], f] += dy[t, f]
// (+ dx[t, :] += dy[t, F:] with cat).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> hip_segment_ext_fwd(
    const torch::Tensor& x, const torch::Tensor& col,
    const torch::Tensor& offsets, int64_t n_tgt, bool is_max, bool cat,
    bool need_arg);
torch::Tensor hip_segment_ext_bwd(const torch::Tensor& dy,
                                  const torch::Tensor& arg, int64_t n_src,
                                  bool cat, bool order_independent);

// --- fused GAT edge softmax + aggregation (hip_gat.hip) ---------------------
// Attention logits are computed inside the kernels from (h, att) directly.
// fwd returns (out, m, Z, s_pre); bwd consumes the cached s_pre logits.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_fused_fwd(
    const torch::Tensor& h_tgt, const torch::Tensor& h_src,
    const torch::Tensor& att_src, const torch::Tensor& att_dst,
    const torch::Tensor& src, const torch::Tensor& offsets, double slope);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_fused_bwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
                  const torch::Tensor& att_src,
                  const torch::Tensor& att_dst, const torch::Tensor& src,
                  const torch::Tensor& offsets, const torch::Tensor& out,
                  const torch::Tensor& m, const torch::Tensor& z,
                  const torch::Tensor& spre, const torch::Tensor& dout,
                  double slope);

// Multi-relation fused GAT: one launch per hetero layer; h views may be
// row-strided slices of the per-type batched projection.  The single entry
// points above are its one-relation case and launch the same kernels.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
hip_gat_multi_fwd(const std::vector<torch::Tensor>& h_tgt,
                  const std::vector<torch::Tensor>& h_src,
                  const std::vector<torch::Tensor>& att_src,
                  const std::vector<torch::Tensor>& att_dst,
                  const std::vector<torch::Tensor>& src,
                  const std::vector<torch::Tensor>& off, double slope,
                  const std::vector<torch::Tensor>& bias);
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
                       double slope);

// --- fused GATv2 attention (hip_gatv2.hip) ----------------------------------
// score_e[h] = sum_c att[h,c] * leaky_relu(h_src[src_e,h,c] + h_tgt[t,h,c]),
// softmax per target segment, out[t] = sum_e p_e * h_src[src_e].  h is fp32
// or bf16, att fp32 [H, C], 1 <= C <= 128; all arguments are validated
// before any launch.  fwd returns (out, m, Z, out_f32); nothing per edge is
// saved.  out_f32 is None unless for_backward; it is the fp32 out the
// backward takes: out itself for fp32 h, the unrounded accumulator for bf16.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor,
           c10::optional<torch::Tensor>>
hip_gatv2_fwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
              const torch::Tensor& att, const torch::Tensor& src,
              const torch::Tensor& offsets, int64_t n_tgt, double slope,
              bool for_backward);
// Atomic-free backward: (dh_tgt, dh_src, datt fp32 [H, C]), dh in h's dtype
// with every row written; out is the forward's out_f32.  dh_src is
// computed, by source, only when (src_off, in_edge) =
// hip_segment_transpose(src, n_src, nullopt) is given, and is None otherwise.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>, torch::Tensor>
hip_gatv2_bwd(const torch::Tensor& h_tgt, const torch::Tensor& h_src,
              const torch::Tensor& att, const torch::Tensor& tgt,
              const torch::Tensor& src, const torch::Tensor& offsets,
              const torch::Tensor& out, const torch::Tensor& m,
              const torch::Tensor& z, const torch::Tensor& dout,
              double slope, const c10::optional<torch::Tensor>& src_off,
              const c10::optional<torch::Tensor>& in_edge);

// --- f32 MFMA projection GEMM (hip_gemm_f32.hip) ----------------------------
torch::Tensor hip_sage_gemm(const torch::Tensor& A, const torch::Tensor& B,
                            const c10::optional<torch::Tensor>& bias,
                            bool relu);

// --- bf16 MFMA projection GEMMs (hip_gemm_bf16.hip) -------------------------
// C = act(A[M,K] @ Bt[N,K]^T + bias): Bt in nn.Linear weight layout.
torch::Tensor hip_gemm_bt_bf16(const torch::Tensor& A,
                               const torch::Tensor& Bt,
                               const c10::optional<torch::Tensor>& bias,
                               bool relu, bool out_fp32);
// The launcher's own dispatch for a shape: the wide BM x 256 kernel, the
// 64x64 kernel or the persistent-B experiment, and the launch grid.
struct GemmBtPlan {
  enum Kernel { NARROW = 0, WIDE = 1, PERSIST = 2 };
  Kernel kernel;
  int64_t grid_x, grid_y;
};
GemmBtPlan gemm_bt_bf16_plan(int64_t M, int64_t K, int64_t N,
                             bool aligned = true);
// Byte offset of a 16-byte chunk in the wide kernel's LDS tile images.
int64_t gemm_bt_tile_offset(int64_t row, int64_t chunk);
// (dW, db) = (A[Kb,M]^T @ B[Kb,N], colsum A), fp32 outputs (split-K).
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> hip_gemm_kt_bf16(
    const torch::Tensor& A, const torch::Tensor& B, bool with_db);
// The launcher's own dispatch for a shape: 128x128 (big) or 64x64 tiles,
// output tile counts, split-K chunks z of k_per_z rows each.
struct GemmKtPlan {
  bool big;
  int64_t m_t, n_t, z, k_per_z;
};
GemmKtPlan gemm_kt_bf16_plan(int64_t Kb, int64_t M, int64_t N);
// Byte offset of a 16-byte chunk in the 128x128 kernel's LDS tile image.
int64_t gemm_kt_tile_offset(int64_t row, int64_t chunk);
torch::Tensor hip_mfma_bf16_selftest(const torch::Tensor& A,
                                     const torch::Tensor& B);

// --- memory plumbing (hip_mem.hip) -----------------------------------------
// Device-dtype alias of (pinned/registered) host memory; keeps `src` alive.
torch::Tensor host_mapped_view(const torch::Tensor& src, int64_t device_index);
// hipHostRegister arbitrary host range (e.g. the shm sample ring).
void pin_host_memory(int64_t addr, int64_t bytes);
void unpin_host_memory(int64_t addr);
void enable_peer_access(int64_t device, int64_t peer);
// IPC sharing of a device tensor: returns handle bytes.
std::string ipc_share(const torch::Tensor& t);
torch::Tensor ipc_open(const std::string& handle, int64_t device,
                       const std::vector<int64_t>& shape,
                       torch::ScalarType dtype);

// --- unified feature store (hip_unified_tensor.hip) ------------------------
class UnifiedFeatureStore;
std::shared_ptr<UnifiedFeatureStore> ufs_create(int64_t device_index);
// Append a row segment; tensor must be HIP-device or a host_mapped_view.
void ufs_append(UnifiedFeatureStore* s, const torch::Tensor& seg);
torch::Tensor ufs_gather(UnifiedFeatureStore* s, const torch::Tensor& rows);
int64_t ufs_rows(UnifiedFeatureStore* s);
int64_t ufs_dim(UnifiedFeatureStore* s);

}  // namespace glt

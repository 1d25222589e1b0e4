"""Autograd wrapper for the fused GAT edge-softmax + aggregation kernels.

The kernels compute the attention logits internally from (h, att), so the
python layer never materializes per-node alpha tensors (saves ~8 small
launches per relation per layer in RGAT's launch-bound regime).

gat_softmax_aggregate / gat_multi_layer: GATv1, fp32-atomic backward.
gatv2_softmax_aggregate: GATv2, atomic-free backward; picks the kernels or
the torch composition (gatv2_composition) itself.
"""
import torch


class _GatFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h_tgt, h_src, att_src, att_dst, src, offsets, slope):
        from .. import _C

        # contiguity once, shared by fwd and the saved tensors bwd reads
        h_tgt = h_tgt.contiguous()
        h_src = h_src.contiguous()
        att_src = att_src.contiguous()
        att_dst = att_dst.contiguous()
        out, m, z, spre = _C.gat_fused_fwd(h_tgt, h_src, att_src, att_dst,
                                           src, offsets, slope)
        ctx.save_for_backward(h_tgt, h_src, att_src, att_dst, src, offsets,
                              out, m, z, spre)
        ctx.slope = slope
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _C

        (h_tgt, h_src, att_src, att_dst, src, offsets, out, m, z,
         spre) = ctx.saved_tensors
        dht, dhs, das, dad = _C.gat_fused_bwd(h_tgt, h_src, att_src,
                                              att_dst, src, offsets, out,
                                              m, z, spre, dout, ctx.slope)
        # kernel accumulates in fp32 arenas; match autograd dtypes
        if dht.dtype != h_tgt.dtype:
            dht = dht.to(h_tgt.dtype)
            dhs = dhs.to(h_src.dtype)
        if das.dtype != att_src.dtype:
            das = das.to(att_src.dtype)
            dad = dad.to(att_dst.dtype)
        return dht, dhs, das, dad, None, None, None


def gat_softmax_aggregate(h_tgt, h_src, att_src, att_dst, tgt, src, n_tgt,
                          negative_slope=0.2):
    """out[t,h,:] = sum_e softmax_t(leaky(<h_tgt[t,h],att_dst[h]> +
    <h_src[src_e,h],att_src[h]>)) * h_src[src_e,h,:], edges sorted by
    target.  att_* are [H, C]."""
    from .segment import _boundaries

    offsets = torch.searchsorted(tgt, _boundaries(n_tgt, tgt.device))
    return _GatFused.apply(h_tgt, h_src, att_src, att_dst,
                           src.contiguous(), offsets, negative_slope)


class _GatV2Fused(torch.autograd.Function):
    """GATv2 attention through the hip_gatv2 kernels.

    Forward saves (out in fp32, m, Z) and nothing per edge; backward
    recomputes the scores.  No gradient is summed with float atomics, so
    all of them are run-to-run identical whatever ``set_deterministic``
    says.
    """

    @staticmethod
    def forward(ctx, h_tgt, h_src, att, tgt, src, offsets, n_tgt, slope):
        from .. import _C

        # contiguity once, shared by fwd and the saved tensors bwd reads
        h_tgt = h_tgt.contiguous()
        h_src = h_src.contiguous()
        att = att.contiguous()
        out, m, z, out_f32 = _C.gatv2_fwd(h_tgt, h_src, att, src, offsets,
                                          n_tgt, slope,
                                          any(ctx.needs_input_grad[:3]))
        ctx.save_for_backward(h_tgt, h_src, att, tgt, src, offsets, out_f32,
                              m, z)
        ctx.slope = slope
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _C

        h_tgt, h_src, att, tgt, src, offsets, out, m, z = ctx.saved_tensors
        # the by-source index is built here, and only for a source
        # projection that wants its gradient (layer 1 of a model whose
        # features need none never pays for it)
        src_off = in_edge = None
        if ctx.needs_input_grad[1]:
            src_off, in_edge = _C.segment_transpose(src, h_src.size(0), None)
        dht, dhs, datt = _C.gatv2_bwd(h_tgt, h_src, att, tgt, src, offsets,
                                      out, m, z, dout.contiguous(),
                                      ctx.slope, src_off, in_edge)
        return dht, dhs, datt, None, None, None, None, None


def gatv2_composition(h_tgt, h_src, att, tgt, src, n_tgt,
                      negative_slope=0.2, dropout=0.0):
    """GATv2 attention as a chain of torch ops: any device, any float
    dtype, any edge order.  It materialises the [E, H, C] pre-activation.

        u_e     = h_src[src_e] + h_tgt[tgt_e]
        score_e = sum_c att[h, c] * leaky_relu(u_e[h, c])
        out[t]  = sum_{e: tgt_e = t} softmax_t(score)_e * h_src[src_e]

    Half-precision inputs are computed in fp32 and the result is returned
    in their dtype.  dropout > 0 drops attention coefficients.
    """
    dtype = h_src.dtype
    if dtype not in (torch.float32, torch.float64):
        h_tgt, h_src = h_tgt.float(), h_src.float()
    att = att.to(h_src.dtype)
    H, C = h_src.size(1), h_src.size(2)
    # index_select (not advanced indexing): its backward is an index_add
    hs = h_src.index_select(0, src)
    u = hs + h_tgt.index_select(0, tgt)
    score = (torch.nn.functional.leaky_relu(u, negative_slope) * att).sum(-1)
    s_max = torch.full((n_tgt, H), float("-inf"), device=score.device,
                       dtype=score.dtype)
    s_max.scatter_reduce_(0, tgt.unsqueeze(1).expand_as(score),
                          score.detach(), reduce="amax", include_self=True)
    # the max is a constant shift of a softmax: no gradient through it
    ex = (score - s_max.index_select(0, tgt)).exp()
    denom = ex.new_zeros(n_tgt, H)
    denom.index_add_(0, tgt, ex)
    alpha = ex / denom.clamp(min=1e-16).index_select(0, tgt)
    if dropout > 0:
        alpha = torch.nn.functional.dropout(alpha, p=dropout)
    out = hs.new_zeros(n_tgt, H, C)
    out.index_add_(0, tgt, hs * alpha.unsqueeze(-1))
    return out.to(dtype)


def gatv2_fused_ok(h_tgt, h_src, sorted_by_target=True) -> bool:
    """Whether gatv2_softmax_aggregate runs the HIP kernels on these."""
    return (sorted_by_target and h_src.is_cuda and h_tgt.is_cuda
            and h_src.dtype in (torch.float32, torch.bfloat16)
            and h_tgt.dtype == h_src.dtype and h_src.dim() == 3
            and 1 <= h_src.size(2) <= 128)


def gatv2_softmax_aggregate(h_tgt, h_src, att, tgt, src, n_tgt,
                            negative_slope=0.2, sorted_by_target=True):
    """GATv2 ("dynamic" attention) edge softmax + aggregation.

    out[t,h,:] = sum_e softmax_t(sum_c att[h,c] * leaky(h_src[src_e,h,c] +
    h_tgt[t,h,c])) * h_src[src_e,h,:].  h_tgt is [>= n_tgt, H, C], h_src
    [n_src, H, C], att [H, C]; a target without edges gets 0.

    GPU fp32 / bf16 inputs with C <= 128 and edges sorted by target run the
    fused kernels (forward, and a backward without float atomics: every
    gradient is bit-reproducible).  Everything else (the CPU, other dtypes,
    C > 128, sorted_by_target=False) runs gatv2_composition.
    """
    if not gatv2_fused_ok(h_tgt, h_src, sorted_by_target):
        return gatv2_composition(h_tgt, h_src, att, tgt, src, n_tgt,
                                 negative_slope)
    from .segment import _offsets

    tgt = tgt.contiguous()
    return _GatV2Fused.apply(h_tgt, h_src, att.float(), tgt,
                             src.contiguous(), _offsets(tgt, n_tgt), n_tgt,
                             negative_slope)


def _multi_unpack(spec, n_rel, n_type, tensors):
    """gat_multi_layer's flat *tensors as (att_src, att_dst, biases,
    h_types, srcs, offs) and the contiguous fp32 [H, C] att lists the
    kernels take."""
    att_src = list(tensors[:n_rel])
    att_dst = list(tensors[n_rel:2 * n_rel])
    biases = list(tensors[2 * n_rel:3 * n_rel])  # empty = no bias
    h_types = list(tensors[3 * n_rel:3 * n_rel + n_type])
    rest = tensors[3 * n_rel + n_type:]
    srcs = list(rest[:n_rel])
    offs = list(rest[n_rel:2 * n_rel])
    H, C = spec["H"], spec["C"]
    as_f = [a.reshape(H, C).float().contiguous() for a in att_src]
    ad_f = [a.reshape(H, C).float().contiguous() for a in att_dst]
    return att_src, att_dst, biases, h_types, srcs, offs, as_f, ad_f


class _GatFusedMulti(torch.autograd.Function):
    """ONE fused attention launch per hetero layer across relations.

    Inputs are the per-TYPE batched projection tensors [N_t, R_t*H*C]
    plus the per-relation attention parameters.  The kernels READ
    contiguous per-relation copies of the projection's column slices;
    only the gradients are strided: the backward emits ONE dh arena per
    type (relations accumulate atomically into their column slices), so
    the per-relation slice-grad zeros/adds disappear entirely.
    """

    @staticmethod
    def forward(ctx, slope, spec, n_rel, n_type, *tensors):
        from .. import _C

        (_, _, biases, h_types, srcs, offs, as_f,
         ad_f) = _multi_unpack(spec, n_rel, n_type, tensors)
        H, C = spec["H"], spec["C"]
        ht_views, hs_views = [], []
        for r in range(n_rel):
            tt, c0t, st, c0s = spec["rels"][r]
            ht = h_types[tt]
            hs = h_types[st]
            # contiguous per-relation h copies for the kernel READS
            # (strided slices of the wide projection measured ~2.5x
            # slower attention kernels); gradients still land in ONE
            # strided arena per type
            ht_views.append(ht[:, c0t:c0t + H * C]
                            .contiguous().view(ht.size(0), H, C))
            hs_views.append(hs[:, c0s:c0s + H * C]
                            .contiguous().view(hs.size(0), H, C))
        b_f = [b.reshape(-1).float().contiguous() for b in biases]
        out, m, z, spre = _C.gat_multi_fwd(ht_views, hs_views, as_f, ad_f,
                                           srcs, offs, slope, b_f)
        ctx.save_for_backward(out, m, z, spre, *tensors)
        ctx.h_views = (ht_views, hs_views)  # contiguous, reused by bwd
        ctx.meta = (slope, spec, n_rel, n_type)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _C

        out, m, z, spre, *tensors = ctx.saved_tensors
        slope, spec, n_rel, n_type = ctx.meta
        (att_src, att_dst, biases, h_types, srcs, offs, as_f,
         ad_f) = _multi_unpack(spec, n_rel, n_type, tensors)
        H, C = spec["H"], spec["C"]
        dh_arenas = [torch.zeros(h.size(), dtype=torch.float32,
                                 device=h.device) for h in h_types]
        das = torch.zeros(n_rel, H, C, dtype=torch.float32,
                          device=out.device)
        dad = torch.zeros_like(das)
        ht_views, hs_views = ctx.h_views
        dht_views, dhs_views = [], []
        for r in range(n_rel):
            tt, c0t, st, c0s = spec["rels"][r]
            ht, hs = h_types[tt], h_types[st]
            dht_views.append(
                dh_arenas[tt][:, c0t:c0t + H * C].view(ht.size(0), H, C))
            dhs_views.append(
                dh_arenas[st][:, c0s:c0s + H * C].view(hs.size(0), H, C))
        _C.gat_multi_bwd(ht_views, hs_views, as_f, ad_f, srcs, offs,
                         out, m, z, spre, dout, dht_views, dhs_views,
                         list(das), list(dad), slope)
        # bias grad via one tree-reduction per biased relation (an
        # in-kernel atomic colsum measured catastrophically contended:
        # every (t, h) wave hits the same H*C floats)
        dsplit = torch.split(dout, [o.numel() - 1 for o in offs], dim=0)
        grads = [das[r].reshape(att_src[r].shape).to(att_src[r].dtype)
                 for r in range(n_rel)]
        grads += [dad[r].reshape(att_dst[r].shape).to(att_dst[r].dtype)
                  for r in range(n_rel)]
        grads += [dsplit[r].float().sum(dim=0).reshape(biases[r].shape)
                  .to(biases[r].dtype) if biases[r].numel() else None
                  for r in range(n_rel)]
        for t in range(n_type):
            grads.append(dh_arenas[t].to(h_types[t].dtype))
        grads.extend([None] * (2 * n_rel))  # srcs, offs
        return (None, None, None, None, *grads)


def gat_multi_layer(slope, spec, att_src_list, att_dst_list, bias_list,
                    h_type_list, src_list, off_list):
    """Run every relation's edge-softmax attention in one launch.

    spec: {"H": heads, "C": channels, "rels": [(tgt_type_idx,
    tgt_col_off, src_type_idx, src_col_off), ...]}.  Returns the
    concatenated
    [sum n_tgt_r, H, C] output arena (split it with torch.split).
    """
    n_rel = len(att_src_list)
    n_type = len(h_type_list)
    return _GatFusedMulti.apply(
        slope, spec, n_rel, n_type,
        *att_src_list, *att_dst_list, *bias_list, *h_type_list,
        *src_list, *off_list)

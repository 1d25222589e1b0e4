"""Dot-product graph attention with edge features (PyG's TransformerConv,
the UniMP layer): the autograd wrapper of the hip_tconv kernels, the torch
composition of the same operation, and the predicate that routes between
them.

    kk_e       = k[src_e] + edge[e]              (edge absent: k[src_e])
    vv_e       = v[src_e] + edge[e]
    score_e[h] = scale * <q[tgt_e, h], kk_e[h]>
    out[t]     = sum_{e: tgt_e = t} softmax_t(score)_e * vv_e    (empty: 0)
"""
import math

import torch


def _dense_rows(x):
    """x with a dense inner [H, C]; its row stride is kept, so a column
    slice of one fused projection output is read in place."""
    if x.numel() == 0 or (x.stride(2) == 1 and x.stride(1) == x.size(2)
                          and (x.size(0) < 2
                               or x.stride(0) >= x.size(1) * x.size(2))):
        return x
    return x.contiguous()


class _TconvFused(torch.autograd.Function):
    """Forward saves (out in fp32, m, Z) and nothing per edge; backward
    recomputes the scores and computes only the gradients that are wanted.
    No gradient is summed with float atomics: all are run-to-run
    identical."""

    @staticmethod
    def forward(ctx, q, k, v, edge, tgt, src, offsets, n_tgt, scale):
        from .. import _C

        q, k, v = _dense_rows(q), _dense_rows(k), _dense_rows(v)
        if edge is not None:
            edge = edge.contiguous()
        out, m, z, out_f32 = _C.tconv_fwd(q, k, v, edge, src, offsets, n_tgt,
                                          scale,
                                          any(ctx.needs_input_grad[:4]))
        ctx.save_for_backward(q, k, v, edge, tgt, src, offsets, out_f32, m, z)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        from .. import _C

        q, k, v, edge, tgt, src, offsets, out, m, z = ctx.saved_tensors
        need_q, need_k, need_v, need_e = ctx.needs_input_grad[:4]
        # the by-source index is built here, and only for a key or value
        # projection that wants its gradient
        src_off = in_edge = None
        if need_k or need_v:
            src_off, in_edge = _C.segment_transpose(src, k.size(0), None)
        dq, dk, dv, dee = _C.tconv_bwd(q, k, v, edge, tgt, src, offsets, out,
                                       m, z, dout.contiguous(), ctx.scale,
                                       need_q, need_e, src_off, in_edge)
        return (dq, dk if need_k else None, dv if need_v else None, dee,
                None, None, None, None, None)


def transformer_attention_composition(q, k, v, tgt, src, n_tgt, edge=None,
                                      scale=None, dropout=0.0):
    """The operation as a chain of torch ops: any device, any float dtype,
    any edge order.  It materialises the gathered keys, values and edge
    embeddings as [E, H, C] tensors.  Half-precision inputs are computed in
    fp32 and the result is returned in their dtype.  dropout > 0 drops
    attention coefficients."""
    dtype = k.dtype
    if dtype not in (torch.float32, torch.float64):
        q, k, v = q.float(), k.float(), v.float()
        edge = None if edge is None else edge.float()
    H, C = k.size(1), k.size(2)
    if scale is None:
        scale = 1.0 / math.sqrt(C)
    # index_select (not advanced indexing): its backward is an index_add
    kk = k.index_select(0, src)
    vv = v.index_select(0, src)
    if edge is not None:
        kk = kk + edge
        vv = vv + edge
    score = (q.index_select(0, tgt) * kk).sum(-1) * scale
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
    out = vv.new_zeros(n_tgt, H, C)
    out.index_add_(0, tgt, vv * alpha.unsqueeze(-1))
    return out.to(dtype)


def transformer_attention_fused_ok(q, k, v, edge=None,
                                   sorted_by_target=True) -> bool:
    """Whether transformer_attention runs the HIP kernels on these."""
    return (bool(sorted_by_target) and k.is_cuda and q.is_cuda and v.is_cuda
            and k.dtype in (torch.float32, torch.bfloat16)
            and q.dtype == k.dtype and v.dtype == k.dtype and k.dim() == 3
            and 1 <= k.size(2) <= 128
            and (edge is None or (edge.is_cuda and edge.dtype == k.dtype)))


def transformer_attention(q, k, v, tgt, src, n_tgt, edge=None, scale=None,
                          sorted_by_target=True):
    """Dot-product attention over a target-grouped edge list.

    q is [>= n_tgt, H, C], k and v [n_src, H, C], edge None or [E, H, C]
    (projected edge features, added to both the key and the value of their
    edge); scale defaults to 1 / sqrt(C).  A target without edges gets 0.

    GPU fp32 / bf16 inputs with C <= 128 and edges sorted by target run the
    fused kernels (forward, and a backward without float atomics that
    computes only the gradients asked for).  Everything else (the CPU,
    other dtypes, C > 128, sorted_by_target=False) runs
    transformer_attention_composition.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(k.size(2))
    if not transformer_attention_fused_ok(q, k, v, edge, sorted_by_target):
        return transformer_attention_composition(q, k, v, tgt, src, n_tgt,
                                                 edge, scale)
    from .segment import _offsets

    tgt = tgt.contiguous()
    return _TconvFused.apply(q, k, v, edge, tgt, src.contiguous(),
                             _offsets(tgt, n_tgt), n_tgt, float(scale))

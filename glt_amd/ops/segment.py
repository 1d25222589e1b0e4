"""Autograd wrappers over the fused HIP segment kernels.

segment_mean / segment_mean_cat: used by SAGEConv when the batch lives on
the GPU and edges are sorted by target (the glt_amd sampler's native edge
order); the layer falls back to torch index_add on CPU or unsorted input.
segment_weighted_sum: GCNConv's aggregation and the edge-weight
primitive; picks the kernels or a torch composition itself.
segment_max / segment_min (+ _cat) and segment_sum: SAGEConv's other
aggregators; they pick the kernels or a torch composition the same way.
"""
import os

import torch

_boundary_cache = {}
_deterministic = False


def set_deterministic(on: bool) -> None:
    """Run-to-run reproducible segment backward (off by default).

    The default backward adds fp32 atomics in whatever order they land,
    so low-order bits differ between runs.  Deterministic mode snaps each
    term to a power-of-two grid below max|dY| so the sums are exact in
    any order (see csrc/hip/hip_segment.hip for the headroom condition).
    It costs precision for terms far below max|dY|: up to 2^-18 max|dY|
    absolute per term.  Also on while
    ``torch.are_deterministic_algorithms_enabled()``.
    """
    global _deterministic
    _deterministic = bool(on)


def is_deterministic() -> bool:
    return _deterministic or torch.are_deterministic_algorithms_enabled()


def _boundaries(n: int, device) -> torch.Tensor:
    """Cached 0..n arange per device (saves one kernel + one python op per
    conv call; the step is launch-bound)."""
    key = (device.type, device.index)
    buf = _boundary_cache.get(key)
    if buf is None or buf.numel() <= n:
        buf = torch.arange(max(n + 1, 1 << 20), device=device)
        _boundary_cache[key] = buf
    return buf[: n + 1]


def _offsets(tgt: torch.Tensor, n_tgt: int) -> torch.Tensor:
    """CSR offsets [n_tgt + 1] of the ascending target ids."""
    return torch.searchsorted(tgt, _boundaries(n_tgt, tgt.device))


def _from_arena(dx, dy):
    """The backward kernels accumulate in an fp32 arena regardless of dy's
    dtype; the gradient (None if not asked for) goes back in dy's."""
    if dx is not None and dx.dtype != dy.dtype:
        dx = dx.to(dy.dtype)
    return dx


def gather_bwd_enabled() -> bool:
    """Whether segment_mean[_cat] take the atomic-free gather backward.
    ``GLT_SEGMENT_BWD=atomic`` (read at every call) keeps the fp32-arena
    atomic backward, for A/B runs and as a fallback."""
    return os.environ.get("GLT_SEGMENT_BWD", "") != "atomic"


def _segment_mean_bwd(ctx, dy, cat):
    """dx of segment_mean / segment_mean_cat.

    Default: the inverted index of col is built here, in backward (a
    layer whose input needs no gradient never pays for it), and one
    gather kernel sums per source row, rounds to dy's dtype and, with
    ``relu_input``, masks by the saved input: no arena, no atomics, no
    separate cast or mask pass.  In deterministic mode the result has
    the bits of the atomic path below; in plain mode it is run-to-run
    identical as well (each source's list keeps the edge order), which
    the atomic path is not.
    """
    from .. import _C

    col, offsets, tgt = ctx.saved_tensors[:3]
    mask = ctx.saved_tensors[3] if ctx.relu_input else None
    dy = dy.contiguous()
    if gather_bwd_enabled():
        src_off, in_tgt = _C.segment_transpose(col, ctx.n_src, tgt)
        fn = _C.segment_mean_cat_bwd_gather if cat \
            else _C.segment_mean_bwd_gather
        return fn(dy, col, offsets, ctx.n_src, is_deterministic(), src_off,
                  in_tgt, mask)
    fn = _C.segment_mean_cat_bwd if cat else _C.segment_mean_bwd
    dx = _from_arena(fn(dy, col, offsets, ctx.n_src, is_deterministic()), dy)
    if mask is not None:
        dx = torch.ops.aten.threshold_backward(dx, mask[:ctx.n_src], 0)
    return dx


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, col, offsets, n_src, tgt, relu_input):
        from .. import _C

        if relu_input:  # x itself is the mask: a reference, no copy
            ctx.save_for_backward(col, offsets, tgt, x)
        else:
            ctx.save_for_backward(col, offsets, tgt)
        ctx.n_src = n_src
        ctx.relu_input = relu_input
        return _C.segment_mean_fwd(x, col, offsets, offsets.numel() - 1)

    @staticmethod
    def backward(ctx, dy):
        return _segment_mean_bwd(ctx, dy, False), None, None, None, None, \
            None


class _SegmentMeanCat(torch.autograd.Function):
    """Fused ``[segment_mean(x) | x[:n_tgt]]`` — one kernel instead of
    segment-mean + dim-1 torch.cat (which costs two full copyBuffer
    passes over [n, F] per conv layer; see profiles/).  Homo-path only:
    targets must be the row prefix of x."""

    @staticmethod
    def forward(ctx, x, col, offsets, n_tgt, tgt, relu_input):
        from .. import _C

        if relu_input:
            ctx.save_for_backward(col, offsets, tgt, x)
        else:
            ctx.save_for_backward(col, offsets, tgt)
        ctx.n_src = x.size(0)
        ctx.relu_input = relu_input
        return _C.segment_mean_cat_fwd(x, col, offsets, n_tgt)

    @staticmethod
    def backward(ctx, dy):
        return _segment_mean_bwd(ctx, dy, True), None, None, None, None, \
            None


def segment_mean(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                 n_tgt: int, relu_input: bool = False) -> torch.Tensor:
    """Mean of x[src[e]] over contiguous tgt segments.

    Requires tgt ascending (glt_amd batches satisfy this); returns
    [n_tgt, F].

    relu_input: x is the output of a ReLU whose own backward was told to
    leave the mask to its consumer (``cast_linear(...,
    relu_grad_by_consumer=True)``); the gradient returned for x is then
    already masked, ``threshold_backward(dx, x, 0)`` (``x <= 0`` is the
    mask of the pre-activation), in the same pass that computes it.
    """
    offsets = _offsets(tgt, n_tgt)
    return _SegmentMean.apply(x.contiguous(), src.contiguous(), offsets,
                              x.size(0), tgt.contiguous(), bool(relu_input))


def segment_mean_cat(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                     n_tgt: int, relu_input: bool = False) -> torch.Tensor:
    """[segment_mean | root] fused: returns [n_tgt, 2F] where the left F
    columns are the neighbor mean and the right F columns are x[:n_tgt].
    relu_input: as in :func:`segment_mean`."""
    offsets = _offsets(tgt, n_tgt)
    return _SegmentMeanCat.apply(x.contiguous(), src.contiguous(), offsets,
                                 n_tgt, tgt.contiguous(), bool(relu_input))


class _SegmentExt(torch.autograd.Function):
    """segment max / min (plain or fused with the root concat) over the
    HIP kernels.  Only ``arg`` is kept for the backward, and only when x
    needs a gradient."""

    @staticmethod
    def forward(ctx, x, col, offsets, n_tgt, is_max, cat):
        from .. import _C

        out, arg = _C.segment_ext_fwd(x, col, offsets, n_tgt, is_max, cat,
                                      ctx.needs_input_grad[0])
        if arg is not None:
            ctx.save_for_backward(arg)
        ctx.n_src = x.size(0)
        ctx.cat = cat
        return out

    @staticmethod
    def backward(ctx, dy):
        from .. import _C

        arg, = ctx.saved_tensors
        dx = _C.segment_ext_bwd(dy.contiguous(), arg, ctx.n_src, ctx.cat,
                                is_deterministic())
        return _from_arena(dx, dy), None, None, None, None, None


def _segment_ext_arg(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                     n_tgt: int, is_max: bool) -> torch.Tensor:
    """int64 [n_tgt, F]: per (target, channel) the source row of the first
    edge, in edge order, that attains the segment extreme; a NaN beats
    every number; -1 for a target without edges.  Torch composition, any
    edge order."""
    E, F = src.numel(), x.size(1)
    arg = torch.full((n_tgt, F), -1, dtype=torch.long, device=x.device)
    if E == 0 or F == 0 or n_tgt == 0:
        return arg
    with torch.no_grad():
        vals = x.index_select(0, src)
        nan = vals.isnan()
        idx = tgt.unsqueeze(1).expand(E, F)
        ext = vals.new_zeros(n_tgt, F).scatter_reduce_(
            0, idx, vals.masked_fill(nan, 0), "amax" if is_max else "amin",
            include_self=False)
        has_nan = vals.new_zeros(n_tgt, F).scatter_reduce_(
            0, idx, nan.to(vals.dtype), "amax", include_self=True) > 0
        hit = torch.where(has_nan[tgt], nan, (vals == ext[tgt]) & ~nan)
        pos = torch.arange(E, device=x.device).unsqueeze(1).expand(E, F)
        first = torch.full((n_tgt, F), E, dtype=torch.long, device=x.device)
        first.scatter_reduce_(0, idx, torch.where(hit, pos, E), "amin",
                              include_self=True)
        found = first < E
        arg = torch.where(found, src[first.clamp(max=E - 1)], arg)
    return arg


def _segment_ext(x, tgt, src, n_tgt, sorted_by_target, is_max, cat):
    if _wsum_fused(x, sorted_by_target):
        return _SegmentExt.apply(x.contiguous(), src.contiguous(),
                                 _offsets(tgt, n_tgt), n_tgt, is_max, cat)
    arg = _segment_ext_arg(x, tgt, src, n_tgt, is_max)
    if x.size(0) == 0:
        out = x.new_zeros(n_tgt, x.size(1))
    else:
        # gather's backward is the gradient rule: one source row per element
        out = torch.where(arg >= 0, x.gather(0, arg.clamp(min=0)),
                          x.new_zeros(()))
    return torch.cat([out, x[:n_tgt]], dim=1) if cat else out


def segment_max(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                n_tgt: int, sorted_by_target: bool = True) -> torch.Tensor:
    """``out[t, f] = max_{e: tgt[e]=t} x[src[e], f]``; returns [n_tgt, F].

    The gradient of ``out[t, f]`` goes to exactly one source row: that of
    the first edge, in edge order, that attains the maximum (the
    torch_scatter rule; torch's ``scatter_reduce`` splits it evenly over
    ties).  The compare is strict and starts from the segment's first
    edge, a NaN in the segment gives NaN (the gradient goes to the first
    NaN edge), a target without edges gets 0 and no gradient.  The result
    is exact: it carries the bits of the winning input.

    GPU fp32/bf16 input with ``sorted_by_target=True`` (tgt ascending, the
    glt_amd batch order) runs the fused HIP kernels: no [E, F] message
    tensor, and an fp32-arena backward that follows ``is_deterministic()``.
    Anything else runs a torch composition with the same semantics.
    """
    return _segment_ext(x, tgt, src, n_tgt, sorted_by_target, True, False)


def segment_min(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                n_tgt: int, sorted_by_target: bool = True) -> torch.Tensor:
    """Minimum counterpart of :func:`segment_max`."""
    return _segment_ext(x, tgt, src, n_tgt, sorted_by_target, False, False)


def segment_max_cat(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                    n_tgt: int,
                    sorted_by_target: bool = True) -> torch.Tensor:
    """[segment_max | root] fused: returns [n_tgt, 2F], the right F columns
    are x[:n_tgt] (targets must be the row prefix of x)."""
    return _segment_ext(x, tgt, src, n_tgt, sorted_by_target, True, True)


def segment_min_cat(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                    n_tgt: int,
                    sorted_by_target: bool = True) -> torch.Tensor:
    """[segment_min | root] fused; see :func:`segment_max_cat`."""
    return _segment_ext(x, tgt, src, n_tgt, sorted_by_target, False, True)


class _SegmentWeightedSum(torch.autograd.Function):
    """out[t] = a[t] * sum_e w[e] * b[col[e]] * x[col[e]] over the HIP
    kernels; w, a, b are fp32 or None.  Gradients for x and w only."""

    @staticmethod
    def forward(ctx, x, w, col, offsets, a, b):
        from .. import _C

        need_dw = w is not None and ctx.needs_input_grad[1]
        # x is kept (and later read) only for the edge-weight gradient
        ctx.save_for_backward(col, offsets, w, a, b, x if need_dw else None)
        ctx.n_src = x.size(0)
        return _C.segment_wsum_fwd(x, col, offsets, w, a, b)

    @staticmethod
    def backward(ctx, dy):
        from .. import _C

        col, offsets, w, a, b, x = ctx.saved_tensors
        need_dx = ctx.needs_input_grad[0]
        need_dw = w is not None and ctx.needs_input_grad[1]
        det = is_deterministic()
        bound = None
        if det and need_dx and col.numel() > 0 and dy.size(0) > 0:
            # terms are bounded by max|dy| * max|a| * max|w| * max|b|
            for f in (w, a, b):
                if f is not None:
                    m = f.abs().amax()
                    bound = m if bound is None else bound * m
        dx, dw = _C.segment_wsum_bwd(dy.contiguous(), x, col, offsets, w, a,
                                     b, ctx.n_src, need_dx, need_dw, det,
                                     bound)
        return _from_arena(dx, dy), dw, None, None, None, None


def _wsum_fused(x: torch.Tensor, sorted_by_target: bool) -> bool:
    """Whether segment_weighted_sum takes the HIP kernels for this input."""
    return bool(sorted_by_target) and x.is_cuda and \
        x.dtype in (torch.float32, torch.bfloat16)


def segment_weighted_sum(x: torch.Tensor, tgt: torch.Tensor,
                         src: torch.Tensor, n_tgt: int,
                         edge_weight: torch.Tensor = None,
                         tgt_scale: torch.Tensor = None,
                         src_scale: torch.Tensor = None,
                         sorted_by_target: bool = True) -> torch.Tensor:
    """``out[t] = tgt_scale[t] * sum_{e: tgt[e]=t} edge_weight[e] *
    src_scale[src[e]] * x[src[e]]``; returns [n_tgt, F].

    edge_weight [E], tgt_scale [n_tgt] and src_scale [x.size(0)] are
    optional (absent = 1) and may be any float dtype.  Gradients flow to x
    and to edge_weight; the scales are constants and must not require
    grad.  GPU fp32/bf16 input with ``sorted_by_target=True`` (tgt
    ascending, the glt_amd batch order) runs the fused HIP kernels:
    atomic-free forward with fp32 accumulation, fp32-arena backward that
    follows ``is_deterministic()``, bit-reproducible edge-weight gradient.
    Anything else runs a torch composition (index_select, mul,
    index_add_).
    """
    for name, s in (("tgt_scale", tgt_scale), ("src_scale", src_scale)):
        if s is not None and s.requires_grad:
            raise ValueError(
                f"segment_weighted_sum: {name} is not differentiable")
    if _wsum_fused(x, sorted_by_target):
        def f32(v):
            return None if v is None else \
                v.to(torch.float32).contiguous()

        offsets = _offsets(tgt, n_tgt)
        a = f32(tgt_scale)
        if a is not None and a.numel() != n_tgt:
            a = a[:n_tgt].contiguous()
        return _SegmentWeightedSum.apply(x.contiguous(), f32(edge_weight),
                                         src.contiguous(), offsets, a,
                                         f32(src_scale))
    msg = x.index_select(0, src)
    if src_scale is not None:
        msg = msg * src_scale.to(x.dtype)[src].unsqueeze(1)
    if edge_weight is not None:
        msg = msg * edge_weight.to(x.dtype).unsqueeze(1)
    out = x.new_zeros(n_tgt, x.size(1))
    out.index_add_(0, tgt, msg)
    if tgt_scale is not None:
        out = out * tgt_scale.to(x.dtype)[:n_tgt].unsqueeze(1)
    return out


def segment_sum(x: torch.Tensor, tgt: torch.Tensor, src: torch.Tensor,
                n_tgt: int, sorted_by_target: bool = True) -> torch.Tensor:
    """``out[t] = sum_{e: tgt[e]=t} x[src[e]]``: segment_weighted_sum
    without factors (same kernels, same fallback)."""
    return segment_weighted_sum(x, tgt, src, n_tgt,
                                sorted_by_target=sorted_by_target)

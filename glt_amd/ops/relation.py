"""Grouped, K-segmented projection for relational (hetero) layers.

    Y_g[i, :] = act( sum over segments s of g with i < M_s of
                     ( x_s[i, :] @ W_s^T + b_s ) )

One call computes every group: the RGCN form of a hetero layer, where the
segments of a node type are its relations' aggregates and its own features.
bf16 device inputs run the grouped MFMA kernels of hip_gemm_grouped.hip
(forward: weight prep + one GEMM launch; backward: mask, input gradients,
weight gradients, fold); everything else runs a torch composition of the
same definition that accumulates in fp32 and rounds once.
"""
from typing import List, Optional, Sequence

import torch


def _check(xs, weights, biases, group, rows):
    """Validates a call and returns N per group (0 for an empty group)."""
    S = len(xs)
    if not (len(weights) == len(biases) == len(group) == S):
        raise ValueError("relation_linear: xs, weights, biases and group "
                         "must have one entry per segment")
    n_of = [0] * len(rows)
    seen = [False] * len(rows)
    for s in range(S):
        x, w, b, g = xs[s], weights[s], biases[s], group[s]
        if not 0 <= g < len(rows):
            raise ValueError("relation_linear: group %d outside rows" % g)
        if x.dim() != 2 or w.dim() != 2 or w.size(1) != x.size(1):
            raise ValueError("relation_linear: x_s [M_s, K_s] and W_s "
                             "[N, K_s] required")
        if x.dtype != xs[0].dtype or x.device != xs[0].device:
            raise ValueError("relation_linear: all xs share one dtype and "
                             "device")
        if w.dtype not in (torch.float32, x.dtype):
            raise ValueError("relation_linear: weights are fp32 or in the "
                             "dtype of xs")
        if b is not None and (b.dtype != torch.float32
                              or b.shape != (w.size(0),)):
            raise ValueError("relation_linear: a bias is fp32 [N]")
        if seen[g] and n_of[g] != w.size(0):
            raise ValueError("relation_linear: N differs inside group %d"
                             % g)
        seen[g], n_of[g] = True, w.size(0)
        if rows[g] < x.size(0):
            raise ValueError("relation_linear: rows[%d] = %d < M_s = %d"
                             % (g, rows[g], x.size(0)))
    return n_of


def relation_linear_uses_kernel(xs: Sequence[torch.Tensor],
                                weights: Sequence[torch.Tensor],
                                group: Sequence[int],
                                rows: Sequence[int]) -> bool:
    """Routing of relation_linear: True when the call runs the grouped HIP
    kernels, False when it runs the torch composition."""
    import os

    if os.environ.get("GLT_DISABLE_BF16_MFMA") or not xs:
        return False
    from .. import _C

    if len(xs) > _C.relation_linear_max_segments() or \
            len(rows) > _C.relation_linear_max_groups():
        return False
    for x, w in zip(xs, weights):
        if not (x.is_cuda and x.dtype == torch.bfloat16 and w.is_cuda):
            return False
        if x.size(1) % 8 != 0 or x.size(1) < 8 or w.size(0) < 1:
            return False
        if x.stride(1) != 1 or (x.size(0) > 1 and x.stride(0) % 8 != 0) \
                or x.data_ptr() % 16 != 0:
            return False
    return True


def _composition(xs, weights, biases, group, rows, relu, n_of):
    """The definition in torch ops: fp32 (or wider) accumulation, one
    rounding to the dtype of xs."""
    dt = xs[0].dtype if xs else torch.float32
    acc_dt = torch.promote_types(dt, torch.float32)
    dev = xs[0].device if xs else None
    accs = [torch.zeros(rows[g], n_of[g], dtype=acc_dt, device=dev)
            for g in range(len(rows))]
    for x, w, b, g in zip(xs, weights, biases, group):
        h = x.to(acc_dt) @ w.to(acc_dt).t()
        if b is not None:
            h = h + b.to(acc_dt)
        m = x.size(0)
        accs[g] = h + accs[g] if m == rows[g] else \
            torch.cat([accs[g][:m] + h, accs[g][m:]], dim=0)
    return [(torch.relu(a) if relu else a).to(dt) for a in accs]


class _RelationLinear(torch.autograd.Function):
    """args = xs + weights + the biases that are present."""

    @staticmethod
    def forward(ctx, group, rows, relu, has_bias, *args):
        from .. import _C

        S = len(group)
        xs = list(args[:S])
        weights = [w.contiguous() for w in args[S:2 * S]]
        present = iter(args[2 * S:])
        empty = xs[0].new_empty(0, dtype=torch.float32)
        biases = [next(present).contiguous() if h else empty
                  for h in has_bias]
        need_t = any(ctx.needs_input_grad[4 + s] for s in range(S))
        w16, wt = _C.relation_linear_prep(weights, need_t)
        ys = _C.relation_linear_fwd(xs, w16, biases, group, rows, relu)
        ctx.group, ctx.has_bias = group, has_bias
        ctx.n_x, ctx.n_t = S, S if need_t else 0
        ctx.w_dtypes = [w.dtype for w in weights]
        ctx.y_shapes = [tuple(y.shape) for y in ys]
        ctx.save_for_backward(*xs, *(wt if need_t else []),
                              *(ys if relu else []))
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        from .. import _C

        S, group = ctx.n_x, ctx.group
        saved = ctx.saved_tensors
        xs, wt = saved[:S], saved[S:S + ctx.n_t]
        ys = list(saved[S + ctx.n_t:])
        # a group whose output nobody used arrives as None
        dys = [xs[0].new_zeros(shape) if dy is None else dy
               for dy, shape in zip(dys, ctx.y_shapes)]
        dym = _C.relation_linear_mask([dy.contiguous() for dy in dys], ys)
        need_x = [s for s in range(S) if ctx.needs_input_grad[4 + s]]
        grads: List[Optional[torch.Tensor]] = [None] * (2 * S)
        if need_x:
            dxs = _C.relation_linear_dgrad(
                dym, [wt[s] for s in need_x], [group[s] for s in need_x],
                [xs[s].size(0) for s in need_x])
            for s, dx in zip(need_x, dxs):
                grads[s] = dx
        # bias gradients in the order the present biases were passed
        b_at, k = {}, 2 * S
        for s in range(S):
            if ctx.has_bias[s]:
                b_at[s], k = k, k + 1
        grads += [None] * (k - 2 * S)
        need_w = [s for s in range(S)
                  if ctx.needs_input_grad[4 + S + s]
                  or (s in b_at and ctx.needs_input_grad[4 + b_at[s]])]
        if need_w:
            with_db = [s in b_at and ctx.needs_input_grad[4 + b_at[s]]
                       for s in need_w]
            dws, dbs = _C.relation_linear_wgrad(
                dym, [xs[s] for s in need_w], [group[s] for s in need_w],
                [dys[group[s]].size(1) for s in need_w], with_db)
            for s, dw, db, wdb in zip(need_w, dws, dbs, with_db):
                if ctx.needs_input_grad[4 + S + s]:
                    grads[S + s] = dw.to(ctx.w_dtypes[s])
                if wdb:
                    grads[b_at[s]] = db
        return (None, None, None, None, *grads)


def relation_linear(xs: Sequence[torch.Tensor],
                    weights: Sequence[torch.Tensor],
                    biases: Sequence[Optional[torch.Tensor]],
                    group: Sequence[int], rows: Sequence[int],
                    relu: bool = False) -> List[torch.Tensor]:
    """Grouped projection: G outputs [rows[g], N_g] in the dtype of xs.

    xs[s] [M_s, K_s]; weights[s] [N_g, K_s] in the nn.Linear layout, fp32
    master parameters or already in the dtype of xs; biases[s] fp32 [N_g]
    or None; group[s] the output of segment s; rows[g] >= every M_s of g.
    A segment covers, and its bias is added on, its first M_s rows only;
    rows no segment covers are act(0).  Zero sizes are legal.  A group
    without segments returns [rows[g], 0].
    """
    xs, weights, biases = list(xs), list(weights), list(biases)
    group, rows = [int(g) for g in group], [int(m) for m in rows]
    n_of = _check(xs, weights, biases, group, rows)
    if not relation_linear_uses_kernel(xs, weights, group, rows):
        return _composition(xs, weights, biases, group, rows, relu, n_of)
    has_bias = [b is not None for b in biases]
    return list(_RelationLinear.apply(
        group, rows, bool(relu), has_bias, *xs, *weights,
        *[b for b in biases if b is not None]))

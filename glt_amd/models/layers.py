"""GNN conv layers over glt_amd sampled batches.

The reference delegates modeling to PyG (reference README.md:279-303);
this image has no PyG, so glt_amd provides the conv layers its examples
and benchmarks need, written against the glt_amd batch convention:
``edge_index[0]`` = target-side (seed) local index, ``edge_index[1]`` =
source/neighbor local index; aggregation flows 1 -> 0.

Dense math lands on hipBLASLt through torch.nn.Linear (or the in-house
MFMA GEMM for skinny shapes); sparse aggregation uses the fused HIP
kernels in csrc/hip/ (segment-mean [+root concat], weighted segment sum,
GAT / GATv2 edge-softmax) on GPU fp32/bf16 batches, with an index_add_ fallback
for CPU/other dtypes.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F


def _degree(target: torch.Tensor, num_nodes: int) -> torch.Tensor:
    return torch.bincount(target, minlength=num_nodes).clamp_(min=1)


class SAGEConv(nn.Module):
    """GraphSAGE conv with a mean (default), max, min or sum aggregator.

    The neighbor- and root-projections live in ONE [out, 2*in] parameter
    applied to [agg | x]: a single GEMM per layer and no per-step weight
    concatenation (the training step is launch-bound; see profiles/).
    Parameter names and shapes do not depend on ``aggr``.

    aggr='max' / 'min' follow the torch_scatter rule: the gradient of an
    output element goes to the one source row of the first edge, in edge
    order, that attains the extreme (see ops.segment_max); a target
    without edges aggregates to 0.  On GPU fp32/bf16 batches sorted by
    target they run the fused HIP kernels, with the [agg | x_root]
    assembly fused in on the homogeneous path.  aggr='sum' runs
    ops.segment_sum followed by torch.cat: there is no fused
    [sum | root] kernel.
    """

    AGGRS = ("mean", "max", "min", "sum")

    def __init__(self, in_channels: int, out_channels: int,
                 root_weight: bool = True, bias: bool = True,
                 aggr: str = "mean"):
        super().__init__()
        if aggr not in self.AGGRS:
            raise ValueError(
                f"SAGEConv: aggr must be one of {self.AGGRS}, got {aggr!r}")
        self.in_channels = in_channels
        self.root_weight = root_weight
        self.aggr = aggr
        self.lin = nn.Linear(2 * in_channels if root_weight else
                             in_channels, out_channels, bias=bias)

    def forward(self, x, edge_index: torch.Tensor,
                num_target: int = None, sorted_by_target: bool = True,
                fuse_relu: bool = False, relu_input: bool = False,
                relu_grad_by_consumer: bool = False) -> torch.Tensor:
        """x: [n, F] or (x_target, x_source) for bipartite relations.
        fuse_relu folds the activation into the projection GEMM epilogue
        (MFMA path); the caller must then skip its own activation.

        relu_input / relu_grad_by_consumer move the ReLU mask of a layer
        boundary from the producer's backward into the consumer's
        (GraphSAGE.forward sets the pair from one predicate).
        relu_input: x is a ReLU output whose producer left its mask to
        this conv; the fused mean aggregation applies it to the gradient
        of x in the pass that computes it.  relu_grad_by_consumer: this
        conv's fused-ReLU projection leaves its mask to the one consumer
        of its output.  A conv that cannot honour a flag on the path it
        takes raises instead of dropping the mask."""
        if relu_input and not self.takes_relu_input(x, sorted_by_target):
            raise ValueError(
                "SAGEConv: relu_input needs the fused mean aggregation "
                "with the gather backward (GPU fp32/bf16 tensor input, "
                "sorted_by_target, aggr='mean', GLT_SEGMENT_BWD unset)")
        if self.aggr != "mean":
            if relu_grad_by_consumer:
                raise ValueError("SAGEConv: relu_grad_by_consumer needs "
                                 "aggr='mean'")
            return self._forward_aggr(x, edge_index, num_target,
                                      sorted_by_target, fuse_relu)
        if isinstance(x, tuple):
            if relu_grad_by_consumer:
                raise ValueError("SAGEConv: relu_grad_by_consumer needs a "
                                 "tensor input")
            x_tgt, x_src = x
            n = num_target if num_target is not None else x_tgt.size(0)
            tgt, src = edge_index[0], edge_index[1]
            if x_src.is_cuda and sorted_by_target and \
                    x_src.dtype in (torch.float32, torch.bfloat16):
                from ..ops import segment_mean

                agg = segment_mean(x_src, tgt, src, n)
            else:
                agg = x_src.new_zeros(n, x_src.size(1))
                agg.index_add_(0, tgt, x_src.index_select(0, src))
                agg = agg / _degree(tgt, n).unsqueeze(1).to(x_src.dtype)
            if self.root_weight:
                xin = torch.cat([agg, x_tgt[:n]], dim=1)
            else:
                xin = agg
            return self._project(xin, fuse_relu=False)
        n = num_target if num_target is not None else x.size(0)
        tgt, src = edge_index[0], edge_index[1]

        if (x.is_cuda and sorted_by_target
                and x.dtype in (torch.float32, torch.bfloat16)):
            # fused wave-per-row segment mean (glt_amd batches are sorted
            # by target local id by construction); with root_weight the
            # kernel also assembles [agg | x[:n]] in place of a dim-1 cat
            if self.root_weight:
                from ..ops import segment_mean_cat

                xin = segment_mean_cat(x, tgt, src, n, relu_input)
            else:
                from ..ops import segment_mean

                xin = segment_mean(x, tgt, src, n, relu_input)
        else:
            agg = x.new_zeros(n, x.size(1))
            agg.index_add_(0, tgt, x.index_select(0, src))
            agg = agg / _degree(tgt, n).unsqueeze(1).to(x.dtype)
            xin = torch.cat([agg, x[:n]], dim=1) if self.root_weight \
                else agg
        return self._project(xin, fuse_relu, relu_grad_by_consumer)

    def takes_relu_input(self, x, sorted_by_target: bool = True) -> bool:
        """Whether forward(x, ...) aggregates through the fused mean
        kernels with the gather backward, the one path that applies a
        ``relu_input`` mask."""
        from ..ops.segment import gather_bwd_enabled

        return (self.aggr == "mean" and isinstance(x, torch.Tensor)
                and x.is_cuda and bool(sorted_by_target)
                and x.dtype in (torch.float32, torch.bfloat16)
                and gather_bwd_enabled())

    def projects_with_cast_relu(self, x) -> bool:
        """Whether forward(x, ..., fuse_relu=True) projects through
        cast_linear, the one projection that can leave its ReLU mask to
        the consumer."""
        return (self.aggr == "mean" and isinstance(x, torch.Tensor)
                and x.dtype != self.lin.weight.dtype)

    def _forward_aggr(self, x, edge_index, num_target, sorted_by_target,
                      fuse_relu):
        """max / min / sum.  The ops take the fused kernels under the
        predicate the mean path uses (GPU, fp32/bf16, sorted_by_target)
        and a torch composition otherwise."""
        from .. import ops

        tgt, src = edge_index[0], edge_index[1]
        bipartite = isinstance(x, tuple)
        if bipartite:
            x_tgt, x_src = x
            fuse_relu = False
        else:
            x_tgt = x_src = x
        n = num_target if num_target is not None else x_tgt.size(0)
        if self.aggr == "sum":
            agg = ops.segment_sum(x_src, tgt, src, n, sorted_by_target)
        elif self.root_weight and not bipartite:
            op = ops.segment_max_cat if self.aggr == "max" \
                else ops.segment_min_cat
            return self._project(op(x_src, tgt, src, n, sorted_by_target),
                                 fuse_relu)
        else:
            op = ops.segment_max if self.aggr == "max" else ops.segment_min
            agg = op(x_src, tgt, src, n, sorted_by_target)
        xin = torch.cat([agg, x_tgt[:n]], dim=1) if self.root_weight \
            else agg
        return self._project(xin, fuse_relu)

    def _project(self, xin, fuse_relu: bool,
                 relu_grad_by_consumer: bool = False):
        from ..ops import cast_linear, mfma_linear, use_mfma_linear

        if xin.dtype != self.lin.weight.dtype:
            # reduced-precision compute over fp32 master params (bf16
            # batches from a bf16 feature store)
            return cast_linear(xin, self.lin.weight, self.lin.bias,
                               relu=fuse_relu,
                               relu_grad_by_consumer=relu_grad_by_consumer)
        if relu_grad_by_consumer:
            raise ValueError("SAGEConv: relu_grad_by_consumer needs the "
                             "cast_linear projection with fuse_relu")
        if use_mfma_linear(xin, self.lin.weight, relu=fuse_relu):
            return mfma_linear(xin, self.lin.weight, self.lin.bias,
                               relu=fuse_relu)
        out = self.lin(xin)
        return F.relu(out) if fuse_relu else out


class GCNConv(nn.Module):
    """GCN with symmetric degree normalization (computed on the sampled
    subgraph)."""

    def __init__(self, in_channels: int, out_channels: int,
                 bias: bool = True):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=bias)

    def forward(self, x, edge_index, num_target: int = None,
                edge_weight: torch.Tensor = None,
                sorted_by_target: bool = False):
        """edge_weight: optional non-negative [E] per-edge weight; the
        degree of a node is then the sum of the weights of its edges
        (either end), nodes of degree 0 get norm 0, and the normalisation
        is a constant (no gradient flows to edge_weight through it).
        sorted_by_target: set True for edges sorted by edge_index[0]
        (loader batches) to run the fused HIP aggregation on the GPU."""
        from .. import ops
        from ..ops.segment import _wsum_fused

        n = x.size(0)
        nt = num_target if num_target is not None else n
        tgt, src = edge_index[0], edge_index[1]
        # the kernels take fp32 factors; the torch path keeps x's dtype
        ndt = torch.float32 if _wsum_fused(x, sorted_by_target) else x.dtype
        if edge_weight is None:
            deg = _degree(torch.cat([tgt, src]), n).to(ndt)
            norm = deg.rsqrt()
        else:
            w = edge_weight.detach().to(
                torch.promote_types(x.dtype, torch.float32))
            deg = w.new_zeros(n)
            deg.index_add_(0, tgt, w)
            deg.index_add_(0, src, w)
            norm = torch.where(deg > 0, deg.rsqrt(),
                               torch.zeros_like(deg)).to(ndt)
        if x.dtype != self.lin.weight.dtype:
            h = ops.cast_linear(x, self.lin.weight, self.lin.bias)
        else:
            h = self.lin(x)
        return ops.segment_weighted_sum(h, tgt, src, nt, edge_weight,
                                        norm[:nt], norm, sorted_by_target)


class GATConv(nn.Module):
    """Multi-head graph attention (GATv1-style, scatter softmax)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1,
                 concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, bias: bool = True):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(
            heads * out_channels if concat else out_channels)) if bias \
            else None
        nn.init.xavier_uniform_(self.att_src)
        nn.init.xavier_uniform_(self.att_dst)

    def forward(self, x, edge_index, num_target: int = None,
                sorted_by_target: bool = True):
        """x: [n, F] or a (x_target, x_source) tuple for bipartite edge
        sets (hetero relations); edge_index[0] indexes the target side,
        edge_index[1] the source side.  sorted_by_target: set False for
        edge sets not sorted by edge_index[0] — the fused segment kernel
        requires ascending targets; the scatter-softmax fallback does
        not."""
        def _proj(v):
            if v.dtype != self.lin.weight.dtype:
                from ..ops import cast_linear

                return cast_linear(v, self.lin.weight, self.lin.bias)
            return self.lin(v)

        if isinstance(x, tuple):
            x_tgt, x_src = x
            nt = num_target if num_target is not None else x_tgt.size(0)
            h_tgt = _proj(x_tgt).view(x_tgt.size(0), self.heads,
                                      self.out_channels)
            h_src = _proj(x_src).view(x_src.size(0), self.heads,
                                      self.out_channels)
        else:
            nt = num_target if num_target is not None else x.size(0)
            h_tgt = h_src = _proj(x).view(x.size(0), self.heads,
                                          self.out_channels)
        return self.attend(h_tgt, h_src, edge_index, nt,
                           sorted_by_target=sorted_by_target)

    def attend(self, h_tgt, h_src, edge_index, nt,
               sorted_by_target: bool = True):
        """Attention + aggregation over pre-projected features
        [n, heads, C] (lets HeteroConv batch the projections of all
        relations sharing a node type into one GEMM)."""
        tgt, src = edge_index[0], edge_index[1]
        h = h_src
        if (sorted_by_target and getattr(self, "use_fused", True)
                and h_src.is_cuda
                and h_src.dtype in (torch.float32, torch.bfloat16)
                and self.out_channels <= 128
                and not (self.training and self.dropout > 0)):
            # fused segment-softmax-aggregate (edges sorted by target);
            # the kernel computes the attention logits itself, so no
            # per-node alpha tensors are built here
            from ..ops import gat_softmax_aggregate

            out = gat_softmax_aggregate(h_tgt, h_src,
                                        self.att_src.squeeze(0),
                                        self.att_dst.squeeze(0),
                                        tgt, src, nt,
                                        self.negative_slope)
            out = out.reshape(nt, self.heads * self.out_channels) \
                if self.concat else out.mean(dim=1)
            if self.bias is not None:
                out = out + self.bias.to(out.dtype)
            return out
        if h_src.dtype != torch.float32:
            h_tgt = h_tgt.float()
            h_src = h = h_src.float()
        alpha_src = (h_src * self.att_src).sum(-1)
        alpha_dst = (h_tgt * self.att_dst).sum(-1)
        # index_select (not advanced indexing): its backward is an
        # index_add scatter, avoiding the radix-sort the indexing backward
        # performs per gather (24 device sorts/step in RGAT otherwise)
        e = alpha_dst.index_select(0, tgt) + alpha_src.index_select(0, src)
        e = F.leaky_relu(e, self.negative_slope)
        # scatter softmax over tgt
        e_max = torch.full((nt, self.heads), float("-inf"),
                           device=e.device, dtype=e.dtype)
        e_max.scatter_reduce_(0, tgt.unsqueeze(1).expand_as(e), e.detach(),
                              reduce="amax", include_self=True)
        # softmax is shift-invariant: the max is a constant offset, so it
        # carries no gradient (and its scatter-amax backward is skipped)
        e = (e - e_max.index_select(0, tgt)).exp()
        denom = torch.zeros(nt, self.heads, device=e.device, dtype=e.dtype)
        denom.index_add_(0, tgt, e)
        alpha = e / denom.clamp(min=1e-16).index_select(0, tgt)
        if self.training and self.dropout > 0:
            alpha = F.dropout(alpha, p=self.dropout)
        msg = h.index_select(0, src) * alpha.unsqueeze(-1)
        out = h.new_zeros(nt, self.heads, self.out_channels)
        out.index_add_(0, tgt, msg)
        out = out.reshape(nt, self.heads * self.out_channels) if self.concat \
            else out.mean(dim=1)
        if self.bias is not None:
            out = out + self.bias
        return out


class GATv2Conv(nn.Module):
    """Multi-head GATv2 ("dynamic" attention, Brody et al. 2022).

    The score of an edge is ``att . leaky_relu(lin_l(x_src) + lin_r(x_tgt))``
    per head, a softmax over each target's edges weighs the messages
    ``lin_l(x_src)``.  Parameter names follow PyG's GATv2Conv (``lin_l``
    source side, ``lin_r`` target side, ``att`` [1, H, C], ``bias``), so
    state dicts port; ``share_weights`` makes ``lin_r`` the same module as
    ``lin_l``.

    GPU fp32 / bf16 batches sorted by target with C <= 128 run the fused
    HIP kernels (ops.gatv2_softmax_aggregate), whose backward has no float
    atomics; everything else, and training with dropout > 0, runs the
    torch composition.  Set ``use_fused = False`` to force the latter.

    Deliberately not a GATConv: HeteroConv sends GATConv relations to the
    v1 multi-relation kernel, GATv2 relations take the per-relation path.
    """

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1,
                 concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, bias: bool = True,
                 share_weights: bool = False):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.share_weights = share_weights
        self.use_fused = True
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else \
            nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(
            heads * out_channels if concat else out_channels)) if bias \
            else None
        for lin in {self.lin_l, self.lin_r}:
            nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        nn.init.xavier_uniform_(self.att)

    def _project(self, lin, v):
        if v.dtype != lin.weight.dtype:
            from ..ops import cast_linear

            h = cast_linear(v, lin.weight, lin.bias)
        else:
            h = lin(v)
        return h.view(v.size(0), self.heads, self.out_channels)

    def forward(self, x, edge_index, num_target: int = None,
                sorted_by_target: bool = True):
        """x: [n, F] with the targets as its first ``num_target`` rows, or
        a (x_target, x_source) tuple for bipartite edge sets;
        edge_index[0] indexes the target side, edge_index[1] the source
        side.  ``lin_r`` only runs over the target rows.
        sorted_by_target: set False for edge sets not sorted by
        edge_index[0]; they take the composition."""
        if isinstance(x, tuple):
            x_tgt, x_src = x
            nt = num_target if num_target is not None else x_tgt.size(0)
            h_src = self._project(self.lin_l, x_src)
            h_tgt = self._project(self.lin_r, x_tgt[:nt])
        else:
            nt = num_target if num_target is not None else x.size(0)
            h_src = self._project(self.lin_l, x)
            h_tgt = h_src[:nt] if self.share_weights \
                else self._project(self.lin_r, x[:nt])
        return self.attend(h_tgt, h_src, edge_index, nt,
                           sorted_by_target=sorted_by_target)

    def attend(self, h_tgt, h_src, edge_index, nt,
               sorted_by_target: bool = True):
        """Attention + aggregation over pre-projected features: h_tgt
        [>= nt, heads, C] from lin_r, h_src [n, heads, C] from lin_l."""
        from ..ops import gatv2_composition, gatv2_softmax_aggregate

        tgt, src = edge_index[0], edge_index[1]
        att = self.att.squeeze(0)
        if self.training and self.dropout > 0:
            # no fused attention dropout
            out = gatv2_composition(h_tgt, h_src, att, tgt, src, nt,
                                    self.negative_slope, self.dropout)
        else:
            out = gatv2_softmax_aggregate(
                h_tgt, h_src, att, tgt, src, nt, self.negative_slope,
                sorted_by_target=sorted_by_target and self.use_fused)
        out = out.reshape(nt, self.heads * self.out_channels) \
            if self.concat else out.mean(dim=1)
        if self.bias is not None:
            out = out + self.bias.to(out.dtype)
        return out

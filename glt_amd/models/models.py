"""Model families exercised by the reference examples: GraphSAGE
(supervised + unsupervised link-pred), GAT, GCN."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers import GATConv, GATv2Conv, GCNConv, SAGEConv


def _layer_trim(num_sampled_nodes, num_sampled_edges, num_layers, layer):
    """Rows/edges needed by layer `layer` (0-based) of an L-layer GNN over a
    glt_amd multi-hop batch: layer l only needs nodes of hops
    0..L-l and edges of hops 1..L-l (hop-ordered concatenation).
    Returns (n_in_rows, n_edges, n_out_rows) or None when trim info is
    unusable."""
    if not num_sampled_nodes or not num_sampled_edges:
        return None
    nsn = [int(v) for v in num_sampled_nodes]
    nse = [int(v) for v in num_sampled_edges]
    L = num_layers
    if len(nse) < L or len(nsn) < L + 1:
        return None
    keep_hops = L - layer          # edges of hops 1..keep_hops
    n_edges = sum(nse[:keep_hops])
    n_in = sum(nsn[:keep_hops + 1])
    n_out = sum(nsn[:keep_hops])
    return n_in, n_edges, n_out


class GraphSAGE(nn.Module):
    def __init__(self, in_channels: int, hidden_channels: int,
                 num_layers: int, out_channels: Optional[int] = None,
                 dropout: float = 0.0, aggr: str = "mean"):
        """aggr: 'mean' | 'max' | 'min' | 'sum', passed to every SAGEConv."""
        super().__init__()
        out_channels = out_channels or hidden_channels
        self.convs = nn.ModuleList()
        dims = ([in_channels] + [hidden_channels] * (num_layers - 1) +
                [out_channels])
        for i in range(num_layers):
            self.convs.append(SAGEConv(dims[i], dims[i + 1], aggr=aggr))
        self.dropout = dropout

    def forward(self, x, edge_index, num_sampled_nodes=None,
                num_sampled_edges=None):
        """Hop-wise trimmed forward: with the per-hop counts from a sampled
        batch, layer l runs only over the rows/edges still reachable from
        the seeds — ~(fan-out) x less compute on the deep layers."""
        L = len(self.convs)
        masked = False  # this layer applies the previous boundary's mask
        for i, conv in enumerate(self.convs):
            act = i < L - 1  # fused into the projection GEMM epilogue
            # one decision per boundary, handed to both of its sides
            defer = act and self._relu_mask_by_consumer(
                x, conv, self.convs[i + 1])
            trim = _layer_trim(num_sampled_nodes, num_sampled_edges, L, i)
            if trim is not None:
                n_in, n_edges, n_out = trim
                x = conv(x[:n_in], edge_index[:, :n_edges],
                         num_target=n_out, fuse_relu=act, relu_input=masked,
                         relu_grad_by_consumer=defer)
            else:
                x = conv(x, edge_index, fuse_relu=act, relu_input=masked,
                         relu_grad_by_consumer=defer)
            masked = defer
            if act:
                x = F.dropout(x, p=self.dropout, training=self.training)
        return x

    def _relu_mask_by_consumer(self, x, conv, nxt) -> bool:
        """Whether the ReLU mask of the boundary conv -> nxt moves from
        conv's projection backward into nxt's aggregation backward, where
        it costs no pass of its own (x is conv's input).

        All of: nxt takes the fused mean aggregation with the gather
        backward (same device and dtype as x: cast_linear returns x's);
        conv projects through cast_linear with the fused ReLU; dropout
        is inactive, so nxt's input IS the ReLU output and ``input <= 0``
        is the pre-activation's mask; nxt is the activation's only
        consumer (forward() hands it to nothing else, and rows nxt trims
        away get zero gradient, which no mask changes).

        forward() evaluates this once per boundary and passes the one
        result to both sides, so the mask cannot be applied twice or not
        at all by a disagreement between them; and a conv that cannot
        honour its flag on the path it actually takes raises (SAGEConv
        .forward) rather than drop the mask.  If GLT_SEGMENT_BWD changes
        between forward and backward, the atomic fallback applies the
        saved mask itself.
        """
        if not isinstance(x, torch.Tensor):
            return False
        if self.training and self.dropout > 0:
            return False
        return conv.projects_with_cast_relu(x) and nxt.takes_relu_input(x)


class GAT(nn.Module):
    def __init__(self, in_channels: int, hidden_channels: int,
                 num_layers: int, out_channels: Optional[int] = None,
                 heads: int = 4, dropout: float = 0.0, v2: bool = False):
        """v2: build GATv2Conv ("dynamic" attention) layers."""
        super().__init__()
        out_channels = out_channels or hidden_channels
        conv = GATv2Conv if v2 else GATConv
        self.convs = nn.ModuleList()
        dim = in_channels
        for i in range(num_layers - 1):
            self.convs.append(conv(dim, hidden_channels, heads=heads))
            dim = hidden_channels * heads
        self.convs.append(conv(dim, out_channels, heads=1, concat=False))
        self.dropout = dropout

    def forward(self, x, edge_index, num_sampled_nodes=None,
                num_sampled_edges=None):
        L = len(self.convs)
        for i, conv in enumerate(self.convs):
            trim = _layer_trim(num_sampled_nodes, num_sampled_edges, L, i)
            if trim is not None:
                n_in, n_edges, n_out = trim
                x = conv(x[:n_in], edge_index[:, :n_edges],
                         num_target=n_out)
            else:
                x = conv(x, edge_index)
            if i < L - 1:
                x = F.elu(x)
                x = F.dropout(x, p=self.dropout, training=self.training)
        return x


class GCN(nn.Module):
    def __init__(self, in_channels: int, hidden_channels: int,
                 num_layers: int, out_channels: Optional[int] = None,
                 dropout: float = 0.0):
        super().__init__()
        out_channels = out_channels or hidden_channels
        self.convs = nn.ModuleList()
        dims = ([in_channels] + [hidden_channels] * (num_layers - 1) +
                [out_channels])
        for i in range(num_layers):
            self.convs.append(GCNConv(dims[i], dims[i + 1]))
        self.dropout = dropout

    def forward(self, x, edge_index, num_sampled_nodes=None,
                num_sampled_edges=None, edge_weight=None,
                sorted_by_target=None):
        """edge_weight: optional non-negative [E] weights aligned with
        edge_index (e.g. ``data.edge_attr[:, 0]`` of a ``with_edge=True``
        loader).  sorted_by_target=None picks the fused aggregation
        exactly when trim lists are given: those only come from the
        loaders, whose batches are target-ascending across hops; a GCN
        called on arbitrary edges keeps the order-agnostic path."""
        L = len(self.convs)
        for i, conv in enumerate(self.convs):
            trim = _layer_trim(num_sampled_nodes, num_sampled_edges, L, i)
            if trim is not None:
                n_in, n_edges, n_out = trim
                x = conv(x[:n_in], edge_index[:, :n_edges],
                         num_target=n_out,
                         edge_weight=None if edge_weight is None
                         else edge_weight[:n_edges],
                         sorted_by_target=True if sorted_by_target is None
                         else sorted_by_target)
            else:
                x = conv(x, edge_index, edge_weight=edge_weight,
                         sorted_by_target=bool(sorted_by_target))
            if i < L - 1:
                x = F.relu(x)
                x = F.dropout(x, p=self.dropout, training=self.training)
        return x


def unsupervised_link_pred_loss(h: torch.Tensor,
                                edge_label_index: torch.Tensor,
                                edge_label: torch.Tensor) -> torch.Tensor:
    """Binary link-prediction loss on embedding dot products (the
    unsupervised GraphSAGE objective)."""
    src = h[edge_label_index[0]]
    dst = h[edge_label_index[1]]
    logits = (src * dst).sum(-1).float()  # bce in fp32 for bf16 runs
    return F.binary_cross_entropy_with_logits(logits, edge_label.float())

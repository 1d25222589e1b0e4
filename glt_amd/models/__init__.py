from .layers import (GATConv, GATv2Conv, GCNConv, SAGEConv,
                     TransformerConv)
from .models import (GAT, GCN, GraphSAGE, GraphTransformer,
                     unsupervised_link_pred_loss)
from .hetero import HeteroConv, RGNN

__all__ = ["GATConv", "GATv2Conv", "GCNConv", "SAGEConv", "TransformerConv",
           "GAT", "GCN", "GraphSAGE", "GraphTransformer",
           "unsupervised_link_pred_loss", "HeteroConv", "RGNN"]

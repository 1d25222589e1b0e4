from .layers import GATConv, GATv2Conv, GCNConv, SAGEConv
from .models import GAT, GCN, GraphSAGE, unsupervised_link_pred_loss
from .hetero import HeteroConv, RGNN

__all__ = ["GATConv", "GATv2Conv", "GCNConv", "SAGEConv", "GAT", "GCN",
           "GraphSAGE", "unsupervised_link_pred_loss", "HeteroConv", "RGNN"]

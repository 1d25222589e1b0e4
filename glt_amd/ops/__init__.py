from .segment import (is_deterministic, segment_mean, segment_mean_cat,
                      segment_weighted_sum, set_deterministic)
from .linear import cast_linear, mfma_linear, use_mfma_linear
from .gat import gat_softmax_aggregate

__all__ = ["segment_mean", "segment_mean_cat", "segment_weighted_sum",
           "set_deterministic",
           "is_deterministic", "cast_linear",
           "mfma_linear", "use_mfma_linear", "gat_softmax_aggregate"]

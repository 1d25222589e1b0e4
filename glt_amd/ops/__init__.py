from .segment import (is_deterministic, segment_max, segment_max_cat,
                      segment_mean, segment_mean_cat, segment_min,
                      segment_min_cat, segment_sum, segment_weighted_sum,
                      set_deterministic)
from .linear import cast_linear, mfma_linear, use_mfma_linear
from .gat import (gat_softmax_aggregate, gatv2_composition,
                  gatv2_softmax_aggregate)

__all__ = ["segment_mean", "segment_mean_cat", "segment_weighted_sum",
           "segment_max", "segment_min", "segment_max_cat",
           "segment_min_cat", "segment_sum",
           "set_deterministic",
           "is_deterministic", "cast_linear",
           "mfma_linear", "use_mfma_linear", "gat_softmax_aggregate",
           "gatv2_softmax_aggregate", "gatv2_composition"]

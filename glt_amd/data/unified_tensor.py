"""Thin python wrapper over the native UnifiedFeatureStore.

Parity: reference python/data/unified_tensor.py (UnifiedTensor wrapper over
csrc UnifiedTensor).  Rows are appended as device segments or host tensors
(auto-mapped); gather dispatches to the wave-per-row HIP kernel.
"""
from typing import List, Optional

import torch


class UnifiedTensor:
    """With quantize='int8' or 'fp8', `dim` is the logical row width, the
    appended tensors are packed rows (ops.quantize_rows) and lookups return
    dequantised rows of `dtype` (bf16 or fp32)."""

    def __init__(self, device: int, dtype: torch.dtype = torch.float32,
                 quantize: Optional[str] = None, dim: Optional[int] = None):
        from .. import _C

        self._C = _C
        self.device = device
        self.dtype = dtype
        self.quantize = quantize
        if quantize is not None:
            assert dim is not None, "a quantised UnifiedTensor needs dim="
            self._store = _C.QuantFeatureStore(device, dim, quantize)
        else:
            self._store = _C.UnifiedFeatureStore(device)
        self._keepalive: List[torch.Tensor] = []

    def append_device_tensor(self, t: torch.Tensor):
        assert t.is_cuda
        self._store.append(t.contiguous())
        self._keepalive.append(t)

    def append_cpu_tensor(self, t: torch.Tensor):
        t = t.contiguous()
        mapped = self._C.host_mapped_view(t, self.device)
        self._store.append(mapped)
        self._keepalive += [t, mapped]

    def __getitem__(self, ids: torch.Tensor) -> torch.Tensor:
        rows = ids.to(torch.device("cuda", self.device), non_blocking=True)
        if self.quantize is not None:
            return self._store.gather(rows, self.dtype)
        return self._store.gather(rows)

    @property
    def shape(self):
        return (self._store.rows(), self._store.dim())

    def size(self, dim: int):
        return self.shape[dim]

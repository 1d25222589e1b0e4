"""8-bit feature rows: the packed format and its definition in plain torch.

A quantised table is a contiguous uint8 [N, S] tensor, S = round_up(F + 4,
16).  Row r holds F codes in bytes [0, F), zero padding in [F, S - 4) and
the row's fp32 scale, little endian, in [S - 4, S).  Codes are 'int8'
(symmetric, [-127, 127]) or 'fp8' (OCP e4m3, torch.float8_e4m3fn, +-448).

`quantize_rows_cpu` and `dequantize_rows` are the definition, one rounded
fp32 operation per line; the HIP kernels (csrc/hip/hip_quant_feature.hip)
give the same bits.
"""
import torch

QMAX = {"int8": 127.0, "fp8": 448.0}
# below this absmax a row is stored as zeros: scale would be subnormal for
# int8 and inv overflow
_AMAX_FLOOR = 2.0 ** -119


def _qmax(fmt: str) -> float:
    if fmt not in QMAX:
        raise ValueError(f"quantised format must be 'int8' or 'fp8', "
                         f"got {fmt!r}")
    return QMAX[fmt]


def packed_stride(dim: int) -> int:
    """Bytes per packed row of `dim` codes."""
    return (dim + 4 + 15) // 16 * 16


def quantize_rows_cpu(x: torch.Tensor, fmt: str,
                      chunk_rows: int = 1 << 16) -> torch.Tensor:
    """Pack a host [N, F] table; chunked over rows, so a large table needs
    no full fp32 copy."""
    q = _qmax(fmt)
    assert x.dim() == 2 and x.size(1) >= 1
    n, dim = x.shape
    s = packed_stride(dim)
    out = torch.zeros(n, s, dtype=torch.uint8)
    for lo in range(0, n, chunk_rows):
        xf = x[lo:lo + chunk_rows].float()
        a = xf.abs()
        amax = torch.where(a.isnan(), 0.0, a).amax(dim=1, keepdim=True)
        live = (amax >= _AMAX_FLOOR) & ~amax.isinf()
        safe = torch.where(live, amax, 1.0)
        # tensor by tensor: a true fp32 division, never a reciprocal multiply
        qt = torch.full_like(safe, q)
        scale = torch.where(live, safe / qt, 0.0)
        inv = qt / safe
        y = xf * inv
        y = torch.where(y.isnan(), 0.0, y).clamp(-q, q)
        if fmt == "int8":
            codes = y.round().to(torch.int8).view(torch.uint8)
        else:
            codes = y.to(torch.float8_e4m3fn).view(torch.uint8)
        rows = out[lo:lo + chunk_rows]
        rows[:, :dim] = torch.where(live, codes, 0)
        rows[:, s - 4:] = scale.contiguous().view(torch.uint8)
    return out


def quantize_rows(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """[N, F] fp32 / bf16 / fp16 -> packed uint8 [N, S] on x's device: the
    HIP kernel for device tensors, the torch twin for host tensors."""
    if x.is_cuda:
        from .. import _C
        return _C.quantize_rows(x.contiguous(), fmt)
    return quantize_rows_cpu(x, fmt)


def dequantize_rows(packed: torch.Tensor, dim: int, fmt: str,
                    out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Packed [n, S] -> [n, dim] in out_dtype: float(code) * scale in fp32,
    then one rounding to out_dtype.  Any device."""
    _qmax(fmt)
    s = packed_stride(dim)
    assert packed.dtype == torch.uint8 and packed.dim() == 2 and \
        packed.size(1) == s
    codes = packed[:, :dim].contiguous()
    if fmt == "int8":
        vals = codes.view(torch.int8).float()
    else:
        vals = codes.view(torch.float8_e4m3fn).float()
    scale = packed[:, s - 4:].contiguous().view(torch.float32)
    return (vals * scale).to(out_dtype)

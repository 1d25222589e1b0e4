"""8-bit feature rows: the packed format and its torch definition against
fp64 bounds (CPU), and the HIP quantiser, gather-dequantise kernel and
Feature(quantize=) against that definition, bit for bit (GPU).

Widths sit at the format's and the layouts' edges: 1 (nearly all padding),
12 (F + 4 == 16), 13 (stride steps to 32), 4 / 7 / 8 (aligned and unaligned
output rows for both output dtypes), 256 / 257 (the quantiser's
register-resident boundary), 300 (several passes), 100 (the flagship).
"""
import functools
import pickle

import pytest
import torch

from glt_amd.ops import (dequantize_rows, packed_stride, quantize_rows,
                         quantize_rows_cpu)
from glt_amd.ops.quant import QMAX

WIDTHS = [1, 4, 7, 8, 12, 13, 100, 256, 257, 300]
FMTS = ["int8", "fp8"]
N = 37
ZERO, NEG_LAST, FLUSHED, KEPT, HAS_NAN, HAS_INF, RAMP = range(7)
U = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def table(F):
    """Seeded normals times a per-row factor 2^-20 .. 2^20; rows 0..6 are
    the special ones."""
    g = torch.Generator().manual_seed(F)
    x = torch.randn(N, F, generator=g) * \
        torch.exp2(torch.linspace(-20, 20, N)).unsqueeze(1)
    sign = torch.where(torch.arange(F) % 2 == 0, 1.0, -1.0)
    x[ZERO] = 0
    x[NEG_LAST, -1] = -2 * x[NEG_LAST].abs().max() - 1
    x[FLUSHED] = sign * 2.0 ** -121
    x[FLUSHED, 0] = 2.0 ** -120
    x[KEPT] = sign * 2.0 ** -119      # codes land on the ties +-63.5 (int8)
    x[KEPT, 0] = 2.0 ** -118
    x[HAS_NAN, F // 2] = float("nan")
    x[HAS_INF, 0] = float("inf")
    # down to 2^-19 of the absmax: fp8 subnormals and underflow to +-0
    x[RAMP] = sign * 3.0 * torch.exp2(-(torch.arange(F) % 20).float())
    return x


@functools.lru_cache(maxsize=None)
def packed_table(F, fmt, dtype=torch.float32):
    return quantize_rows_cpu(table(F).to(dtype), fmt)


def error_bound(x64, scale64, fmt):
    """|x - dq| bound that follows from the definition; u absorbs the fp32
    roundings of scale, inv and the products."""
    if fmt == "int8":
        return (0.5 + 4 * U * QMAX[fmt]) * scale64
    return torch.maximum(x64.abs() * 2.0 ** -4,
                         scale64 * 2.0 ** -10) * (1 + 2.0 ** -12)


def scales(packed):
    return packed[:, -4:].contiguous().view(torch.float32)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("F", WIDTHS)
def test_cpu_definition(F, fmt):
    x, p = table(F), packed_table(F, fmt)
    S = packed_stride(F)
    assert S == (F + 4 + 15) // 16 * 16 and p.shape == (N, S)
    assert p.dtype == torch.uint8 and not p[:, F:S - 4].any()
    a = x.abs()
    amax = torch.where(a.isnan(), 0.0, a).amax(dim=1, keepdim=True)
    live = (amax >= 2.0 ** -119) & ~amax.isinf()
    want = torch.where(live, amax / torch.full_like(amax, QMAX[fmt]), 0.0)
    assert torch.equal(scales(p), want)
    assert not p[~live.squeeze(1)].any()        # flushed rows: all zero
    assert live[KEPT] and not live[FLUSHED] and not live[HAS_INF]
    assert not live[ZERO] and (F == 1 or live[HAS_NAN])
    assert p[HAS_NAN, F // 2] == 0
    dq = dequantize_rows(p, F, fmt, torch.float32).double()
    ok = live & ~x.isnan()
    err = (torch.where(ok, x, 0.0).double() - torch.where(ok, dq, 0.0)).abs()
    bound = error_bound(torch.where(ok, x, 0.0).double(),
                        scales(p).double(), fmt)
    assert (err <= bound).all(), float((err - bound).max())
    if fmt == "int8":
        assert (err <= amax.double() / 254 * (1 + 2.0 ** -12)).all()
        codes = p[:, :F].view(torch.int8)
        assert codes.min() >= -127 and codes[NEG_LAST, -1] == -127
        if F > 1:                               # ties go to even
            assert codes[KEPT, 1] == -64 and codes[KEPT, F - 1] in (64, -64)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16,
                                   torch.float16])
@pytest.mark.parametrize("F", WIDTHS)
def test_quantize_rows_kernel(F, dtype, fmt):
    x = table(F).to(dtype)
    got = quantize_rows(x.cuda(), fmt).cpu()
    want = packed_table(F, fmt, dtype)
    diff = (got != want)
    assert torch.equal(got, want), (int(diff.sum()), diff.nonzero()[:8])


def three_tier_store(p, F, fmt):
    from glt_amd import _C
    store = _C.QuantFeatureStore(0, F, fmt)
    mapped = _C.host_mapped_view(p[10:25].contiguous().pin_memory(), 0)
    for seg in (p[:10].cuda(), mapped, p[25:].cuda()):
        store.append(seg)
    return store


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("F", WIDTHS)
def test_gather_dequant_kernel(F, out_dtype, fmt):
    p = packed_table(F, fmt)
    store = three_tier_store(p, F, fmt)
    assert store.rows() == N and store.dim() == F
    g = torch.Generator().manual_seed(1)
    rows = torch.cat([torch.tensor([0, 9, 10, 24, 25, 36, 36, 10, 0, 9]),
                      torch.randint(0, N, (50,), generator=g)])
    got = store.gather(rows.cuda(), out_dtype)
    want = dequantize_rows(p[rows], F, fmt, out_dtype)
    assert got.dtype == out_dtype and got.shape == (rows.numel(), F)
    bits = torch.int16 if out_dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.cpu().view(bits), want.view(bits))   # -0 too


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_gather_single_segment_and_empty(fmt):
    from glt_amd import _C
    F = 100
    p = packed_table(F, fmt)
    store = _C.QuantFeatureStore(0, F, fmt)
    store.append(p.cuda())
    rows = torch.arange(N - 1, -1, -1)
    assert torch.equal(store.gather(rows.cuda(), torch.bfloat16).cpu(),
                       dequantize_rows(p[rows], F, fmt, torch.bfloat16))
    out = store.gather(torch.empty(0, dtype=torch.int64, device="cuda"),
                       torch.float32)
    assert out.shape == (0, F) and out.dtype == torch.float32


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_feature_quantized(fmt):
    from glt_amd.data import Feature
    F = 100
    x = table(F)[RAMP:].contiguous()            # finite rows only
    ids = torch.tensor([0, 5, len(x) - 1, 14, 15, 16, 5, 29])
    f = Feature(x, split_ratio=0.5, device=0, quantize=fmt)
    host = Feature(x, with_gpu=False, quantize=fmt)
    got = f[ids]
    assert f.shape == (len(x), F) and f.size(1) == F
    assert f.dtype == torch.bfloat16 and got.dtype == torch.bfloat16
    assert f.storage_bytes_per_row == packed_stride(F) == 112
    assert 0 < f.device_rows < len(x)
    assert torch.equal(got.cpu(), host[ids])
    assert torch.equal(got.cpu(), f.cpu_get(ids))
    f32 = Feature(x, split_ratio=0.5, device=0, quantize=fmt,
                  dequant_dtype=torch.float32)
    err = (x[ids].double() - f32[ids].cpu().double()).abs()
    sc = scales(f32.cpu_tensor[ids]).double()
    assert (err <= error_bound(x[ids].double(), sc, fmt)).all()
    again = Feature.from_ipc(f.share_ipc())
    assert again.shape == f.shape and again.dtype == f.dtype
    assert torch.equal(again[ids], got)
    assert torch.equal(pickle.loads(pickle.dumps(host))[ids], host[ids])


@pytest.mark.gpu
def test_argument_checks():
    from glt_amd import _C
    F = 12
    p = packed_table(F, "int8").cuda()
    rows = torch.zeros(3, dtype=torch.int64, device="cuda")
    store = _C.QuantFeatureStore(0, F, "int8")
    with pytest.raises(RuntimeError):
        store.gather(rows, torch.float32)       # empty store
    store.append(p)
    bad_segments = [p.float(), p[0], p.t().contiguous().t(), p.cpu(),
                    torch.cat([p, p], dim=1)]
    for seg in bad_segments:
        with pytest.raises(RuntimeError):
            store.append(seg)
    assert store.rows() == N
    for bad_rows, dt in [(rows.int(), torch.float32),
                         (rows.cpu(), torch.float32),
                         (rows, torch.float16)]:
        with pytest.raises(RuntimeError):
            store.gather(bad_rows, dt)
    with pytest.raises(RuntimeError):
        _C.QuantFeatureStore(0, F, "int4")
    with pytest.raises(RuntimeError):
        _C.quantize_rows(table(F).cuda(), "e5m2")
    for _ in range(15):
        store.append(p)
    with pytest.raises(RuntimeError):
        store.append(p)                         # a 17th segment
    assert store.rows() == 16 * N

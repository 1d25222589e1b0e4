"""Order-independent backward kernels: in deterministic mode (off by
default) the segment-mean backward snaps every term to a power-of-two
grid q before its fp32 atomicAdd, so partial sums are exact and
run-to-run results are bit-identical; the default mode keeps plain fp32
accuracy per element.  The bf16 GEMM's bias gradient is always folded
from per-chunk rows in a fixed order.

Bounds used below (H = 6 headroom bits, as kGridHeadroomBits):
  amax = max|dy|, 2^(e-1) <= amax < 2^e, q = 2^(e + H - 24)
  per term: |snap(v) - v| <= q/2, plus one fp32 rounding of dy * (1/deg)
            (<= 2^-23 amax, two roundings of a value <= amax)
  per dx element with cnt terms: cnt * (q/2 + 2^-23 amax), and nothing
  else while |partial sums| < 2^24 q = 2^H 2^e (exact adds).
"""
import math

import pytest
import torch

from glt_amd import _C

pytestmark = pytest.mark.gpu

H = 6


def _graph(n_tgt, n_src, deg, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    tgt = torch.arange(n_tgt, device="cuda").repeat_interleave(deg)
    col = torch.randint(0, n_src, (n_tgt * deg,), device="cuda", generator=g)
    off = torch.arange(0, n_tgt * deg + 1, deg, device="cuda")
    return tgt, col, off


def _ref_bwd(dy, tgt, col, deg, n_src, cat):
    """fp64 reference + number of terms per dx row."""
    d = dy.double()
    F = d.size(1) // 2 if cat else d.size(1)
    ref = torch.zeros(n_src, F, dtype=torch.float64, device="cuda")
    ref.index_add_(0, col, d[tgt, :F] / deg)
    cnt = torch.bincount(col, minlength=n_src).double()
    if cat:
        ref[:d.size(0)] += d[:, F:]
        cnt[:d.size(0)] += 1
    return ref, cnt


def _q(amax):
    e = math.frexp(amax)[1]
    return 2.0 ** (e + H - 24)


def _wide_dy(rows, cols, dtype, seed):
    """Values spread over six decades, like real activation gradients."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (-6.0 * torch.rand(rows, cols, device="cuda", generator=g))
    return (torch.randn(rows, cols, device="cuda", generator=g) * mag).to(
        dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cat", [False, True])
def test_segment_bwd_bit_reproducible_and_bounded(dtype, cat):
    # ~20 atomics from different waves per dx element, several blocks,
    # F not a multiple of the wave; sums stay far below the headroom
    n_tgt, n_src, deg, F = 4000, 4100, 10, 130
    tgt, col, off = _graph(n_tgt, n_src, deg, 0)
    dy = _wide_dy(n_tgt, 2 * F if cat else F, dtype, 1)
    fn = _C.segment_mean_cat_bwd if cat else _C.segment_mean_bwd
    runs = [fn(dy, col, off, n_src, True) for _ in range(3)]
    assert runs[0].dtype == torch.float32 and runs[0].shape == (n_src, F)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])

    ref, cnt = _ref_bwd(dy, tgt, col, deg, n_src, cat)
    amax = dy.float().abs().max().item()
    bound = cnt * (_q(amax) / 2 + 2.0 ** -23 * amax)
    err = (runs[0].double() - ref).abs()
    print("max err %.3e, max bound %.3e, amax %.3e" % (
        err.max().item(), bound.max().item(), amax))
    assert (err <= bound.unsqueeze(1)).all()


def test_segment_bwd_beyond_headroom_is_plain_fp32():
    """A hub row collecting far more than 2^H * max|dy| loses exactness
    (and with it reproducibility) but not accuracy: the error stays within
    the plain sequential fp32 summation bound (n-1) * 2^-24 * sum|terms|
    plus the snap bound."""
    n_tgt, n_src, F = 4096, 4096, 64
    tgt = torch.arange(n_tgt, device="cuda")
    col = torch.zeros(n_tgt, dtype=torch.long, device="cuda")  # all -> row 0
    off = torch.arange(n_tgt + 1, device="cuda")
    dy = 1.0 + 0.5 * torch.rand(n_tgt, F, device="cuda")
    dx = _C.segment_mean_bwd(dy, col, off, n_src, True)
    ref = dy.double().sum(0)
    amax = dy.abs().max().item()
    assert ref.min().item() > 2 ** H * amax * 2  # really past the headroom
    bound = (n_tgt - 1) * 2.0 ** -24 * dy.double().abs().sum(0) \
        + n_tgt * (_q(amax) / 2)
    err = (dx[0].double() - ref).abs()
    print("max err %.3e, min bound %.3e" % (err.max().item(),
                                            bound.min().item()))
    assert (err <= bound).all()
    assert not dx[1:].any()


def test_segment_bwd_edge_cases():
    n_tgt, n_src, deg, F = 70, 90, 3, 33
    tgt, col, off = _graph(n_tgt, n_src, deg, 2)
    # all-zero dy: no grid, exact zeros
    z = _C.segment_mean_bwd(torch.zeros(n_tgt, F, device="cuda"), col, off,
                            n_src, True)
    assert z.shape == (n_src, F) and not z.any()
    # a non-finite entry switches snapping off; it must reach its rows and
    # nothing else, and every other element keeps plain fp32 accuracy
    dy = torch.randn(n_tgt, F, device="cuda")
    dy[5, 7] = float("inf")
    dx = _C.segment_mean_bwd(dy, col, off, n_src, True)
    hit = torch.zeros(n_src, F, dtype=torch.bool, device="cuda")
    hit[col[5 * deg:6 * deg], 7] = True
    assert torch.isinf(dx[hit]).all() and torch.isfinite(dx[~hit]).all()
    dyf = dy.clone()
    dyf[5, 7] = 0.0
    ref, cnt = _ref_bwd(dyf, tgt, col, deg, n_src, False)
    # cnt term roundings (2^-23 amax each) + sequential fp32 summation of
    # cnt terms of at most amax: (cnt-1) * 2^-24 * cnt * amax
    bound = ((cnt * 2.0 ** -23 + cnt * cnt * 2.0 ** -24)
             * dyf.abs().max().item()).unsqueeze(1)
    assert ((dx.double() - ref).abs()[~hit] <= bound.expand_as(ref)[~hit]
            ).all()
    # tiny amax: q would leave the normal range -> no snapping, exact terms
    tiny = torch.full((n_tgt, F), 2.0 ** -120, device="cuda")
    dt = _C.segment_mean_bwd(tiny, col, off, n_src, True)
    reft, _ = _ref_bwd(tiny, tgt, col, deg, n_src, False)
    assert torch.allclose(dt.double(), reft, rtol=1e-5, atol=0.0)
    # no targets at all
    e = _C.segment_mean_bwd(torch.zeros(0, F, device="cuda"),
                            col[:0], off[:1], n_src, True)
    assert e.shape == (n_src, F) and not e.any()
    ec = _C.segment_mean_cat_bwd(torch.zeros(0, 2 * F, device="cuda"),
                                 col[:0], off[:1], n_src, True)
    assert ec.shape == (n_src, F) and not ec.any()


@pytest.mark.parametrize("cat", [False, True])
def test_segment_bwd_default_keeps_fp32_accuracy_per_element(cat):
    """Default (plain) mode: each dx element is accurate relative to ITS
    OWN terms, however far below max|dy| they are: cnt terms with two
    roundings each plus sequential fp32 summation stay within
    (cnt + 2) * 2^-24 * sum|terms|."""
    n_tgt, n_src, deg, F = 4000, 4100, 10, 130
    tgt, col, off = _graph(n_tgt, n_src, deg, 4)
    dy = _wide_dy(n_tgt, 2 * F if cat else F, torch.float32, 5)
    fn = _C.segment_mean_cat_bwd if cat else _C.segment_mean_bwd
    dx = fn(dy, col, off, n_src)
    ref, cnt = _ref_bwd(dy, tgt, col, deg, n_src, cat)
    mag, _ = _ref_bwd(dy.abs(), tgt, col, deg, n_src, cat)
    bound = (cnt.unsqueeze(1) + 2) * 2.0 ** -24 * mag
    assert ((dx.double() - ref).abs() <= bound).all()


def test_deterministic_switch_routes_autograd():
    from glt_amd.ops import (is_deterministic, segment_mean_cat,
                             set_deterministic)

    assert not is_deterministic()
    n_tgt, n_src, deg, F = 2000, 2100, 10, 64
    tgt, col, _ = _graph(n_tgt, n_src, deg, 6)
    x = torch.randn(n_src, F, device="cuda")
    g = _wide_dy(n_tgt, 2 * F, torch.float32, 7)

    def grad():
        xx = x.clone().requires_grad_(True)
        segment_mean_cat(xx, tgt, col, n_tgt).backward(g)
        return xx.grad

    plain = grad()
    set_deterministic(True)
    try:
        assert is_deterministic()
        a, b = grad(), grad()
    finally:
        set_deterministic(False)
    assert torch.equal(a, b)
    # the two modes differ by at most the snap bound
    ref_cnt = torch.bincount(col, minlength=n_src).double()
    ref_cnt[:n_tgt] += 1
    amax = g.abs().max().item()
    bound = (ref_cnt * (_q(amax) + 2.0 ** -21 * amax)).unsqueeze(1)
    assert ((a.double() - plain.double()).abs() <= bound).all()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert is_deterministic()
    finally:
        torch.use_deterministic_algorithms(False)
    assert not is_deterministic()


def test_gemm_kt_db_bit_reproducible():
    """Bias gradient over many split-K chunks (both tile variants): same
    bits every call, and within the fp32 summation bound of the fp64
    column sums (bf16 inputs are exact in fp64)."""
    torch.manual_seed(3)
    for Kb, M, N in [(20_000, 256, 200), (5000, 47, 512)]:
        A = torch.randn(Kb, M, device="cuda").to(torch.bfloat16)
        B = torch.randn(Kb, N, device="cuda").to(torch.bfloat16)
        outs = [_C.gemm_kt_bf16(A, B, True) for _ in range(3)]
        for C, db in outs[1:]:
            assert torch.equal(db, outs[0][1]) and torch.equal(C, outs[0][0])
        db = outs[0][1]
        assert db.shape == (M,) and db.dtype == torch.float32
        ref = A.double().sum(0)
        bound = Kb * 2.0 ** -24 * A.double().abs().sum(0)
        assert ((db.double() - ref).abs() <= bound).all()

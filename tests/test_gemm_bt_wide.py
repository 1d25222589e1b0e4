"""gemm_bt_wide: the 64 x 256 forward tile, its swizzled LDS image, the
plan that chooses between it and the 64x64 gemm_bt kernel, and bit identity
of the two.

A. Plan and layout, without a GPU.  `_C.gemm_bt_bf16_plan(M, K, N)` is the
   launcher's own dispatch.  `_C.gemm_bt_tile_offset(row, chunk)` is the one
   function the kernel stores and reads its staged tiles through: the byte
   offset of 16-byte chunk `chunk` (k = 8*chunk .. 8*chunk+7) of row `row`
   of a [rows][64] bf16 image (64 rows of A, 256 of Bt).  The tests form
   the addresses the kernel's lanes form and check them against the LDS
   rules of the hardware: a 16-byte store is banked by (addr / 4) % 32 over
   each group of 8 consecutive lanes; a 16-byte read by (addr / 4) % 64
   over four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
   and the same two shifted by 32.

B. On the GPU, with GLT_GEMM_BT=wide so that small M reaches the kernel:
   exact integer arithmetic and the derived bounds of test_gemm_family
   (whose helpers this file imports), and `torch.equal` between the wide
   and the 64x64 kernel on real-valued input, which pins "same operands,
   same order".  The grid is neither capped nor persistent (one workgroup
   per tile), so there is no stride loop to wrap.
"""
import pytest
import torch

from glt_amd import _C

from test_gemm_family import (BF16, COMBOS, _assert_bounded, _bound,
                              _bt_case, _ints, _rounding_stats,
                              _run_bt_exact)

ROWS_A, ROWS_B, CHUNKS = 64, 256, 8


def _plan(M, K, N, **kw):
    return _C.gemm_bt_bf16_plan(M, K, N, **kw)


# --------------------------------------------------------------------------
# A. plan and layout (CPU)
# --------------------------------------------------------------------------
def test_plan_table(monkeypatch):
    monkeypatch.delenv("GLT_GEMM_BT", raising=False)
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    # flagship L0, L1 forward, L1 input gradient
    assert _plan(166000, 200, 256) == ("wide", 2594, 1)
    assert _plan(16300, 512, 256) == ("wide", 255, 1)
    assert _plan(16300, 256, 512) == ("wide", 510, 1)
    # K % 8 != 0 or N < 128: the 64x64 kernel, on its 2-D grid
    assert _plan(1024, 47, 512) == ("narrow", 16, 8)
    assert _plan(257, 129, 200) == ("narrow", 5, 4)
    assert _plan(64, 64, 64) == ("narrow", 1, 1)
    # the measured M threshold: 192 row tiles of 64
    assert _plan(12288, 512, 256) == ("wide", 192, 1)
    assert _plan(12287, 512, 256) == ("narrow", 192, 4)
    # every other precondition, one at a time
    assert _plan(16300, 24, 256)[0] == "narrow"          # K < 32
    assert _plan(16300, 32, 128)[0] == "wide"
    assert _plan(16300, 32, 127)[0] == "narrow"
    assert _plan(16300, 200, 256, aligned=False)[0] == "narrow"


def test_plan_override_moves_the_m_threshold_only(monkeypatch):
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    monkeypatch.delenv("GLT_GEMM_BT", raising=False)
    assert _plan(129, 200, 256)[0] == "narrow"           # M below threshold
    monkeypatch.setenv("GLT_GEMM_BT", "wide")
    assert _plan(129, 200, 256) == ("wide", 3, 1)
    assert _plan(130, 256, 512) == ("wide", 6, 1)        # 3 row x 2 col
    assert _plan(1, 32, 128) == ("wide", 1, 1)
    assert _plan(257, 129, 200)[0] == "narrow"           # cannot take wide
    assert _plan(129, 200, 256, aligned=False)[0] == "narrow"
    monkeypatch.setenv("GLT_GEMM_BT", "narrow")
    assert _plan(166000, 200, 256) == ("narrow", 2594, 4)
    monkeypatch.setenv("GLT_GEMM_BT", "sideways")
    with pytest.raises(RuntimeError):
        _plan(129, 200, 256)


def test_plan_persist_keeps_precedence(monkeypatch):
    monkeypatch.setenv("GLT_GEMM_PERSIST", "1")
    monkeypatch.setenv("GLT_GEMM_BT", "wide")
    assert _plan(66000, 40, 128) == ("persist", 1024, 2)
    assert _plan(166000, 200, 256)[0] == "persist"
    assert _plan(16300, 512, 256)[0] == "wide"           # K > 256


def test_plan_degenerate_sizes(monkeypatch):
    """Zero sizes divide by nothing; the launcher returns before it plans
    when M or N is 0, and K = 0 stays on the 64x64 kernel."""
    for force in (None, "wide"):
        if force is None:
            monkeypatch.delenv("GLT_GEMM_BT", raising=False)
        else:
            monkeypatch.setenv("GLT_GEMM_BT", force)
        for shape in [(0, 16, 5), (5, 16, 0), (0, 0, 0), (5, 0, 0),
                      (0, 200, 256), (166000, 200, 0), (166000, 0, 256)]:
            assert _plan(*shape)[0] == "narrow", shape


def _off(row, ch):
    return _C.gemm_bt_tile_offset(row, ch)


def _max_per_bank(accesses, n_banks):
    """accesses: (byte address, bytes) of the lanes of one group.  The
    largest number of distinct addresses that touch one bank."""
    banks = {}
    for addr, size in set(accesses):
        for d in range(size // 4):
            banks.setdefault((addr // 4 + d) % n_banks, set()).add(addr)
    return max(len(v) for v in banks.values())


def test_tile_offset_is_a_bijection_of_aligned_chunks():
    for rows in (ROWS_A, ROWS_B):   # the A image is a prefix of the rule
        offs = sorted(_off(r, ch) for r in range(rows)
                      for ch in range(CHUNKS))
        assert offs == list(range(0, rows * 128, 16))


def test_tile_offset_rejects_out_of_range():
    for row, ch in [(-1, 0), (256, 0), (0, -1), (0, 8)]:
        with pytest.raises(RuntimeError):
            _C.gemm_bt_tile_offset(row, ch)


def test_staging_writes_are_conflict_free():
    """Thread tid stores chunk tid & 7 of row (tid >> 3) + 32 h.  A 16-byte
    store is served in groups of 8 consecutive lanes, banks
    (addr / 4) % 32: every group covers the 32 banks exactly once."""
    for tid0 in range(0, 256, 8):
        for h in range(ROWS_B // 32):
            acc = [(_off((tid >> 3) + 32 * h, tid & 7), 16)
                   for tid in range(tid0, tid0 + 8)]
            assert _max_per_bank(acc, 32) == 1, (tid0, h)


READ_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
]
READ_GROUPS += [[l + 32 for l in grp] for grp in READ_GROUPS]


def test_fragment_reads_are_conflict_free():
    """Lane l of a wave reads chunk kk / 8 + (l >> 4) of row base + (l & 15)
    for every aligned 16-row block `base` and kk in {0, 32}.  Each of the
    four 16-lane groups of a 16-byte read covers the 64 banks once."""
    assert sorted(l for grp in READ_GROUPS for l in grp) == list(range(64))
    for base in range(0, ROWS_B, 16):
        for kk in (0, 32):
            for grp in READ_GROUPS:
                acc = [(_off(base + (l & 15), kk // 8 + (l >> 4)), 16)
                       for l in grp]
                assert _max_per_bank(acc, 64) == 1, (base, kk, grp)


def test_unswizzled_layout_conflicts_by_the_same_rule():
    """The rule has teeth: plain 128-byte rows read 4-way."""
    acc = [(128 * (l & 15) + 16 * (l >> 4), 16) for l in READ_GROUPS[0]]
    assert _max_per_bank(acc, 64) == 4


# --------------------------------------------------------------------------
# B. on the GPU
# --------------------------------------------------------------------------
def _force(monkeypatch, which):
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    monkeypatch.setenv("GLT_GEMM_BT", which)


# (M, K, N, lowest input value, asserts that bf16 rounding is exercised)
WIDE_EXACT = [
    (1, 32, 128, -3, False),
    (129, 200, 256, -3, False),     # M tail, K tail of 8
    (64, 40, 129, -3, False),       # N tail of one column, unaligned rows
    (257, 512, 256, -3, False),
    (130, 256, 512, -3, False),     # two column blocks
    (70, 2000, 136, -3, True),
    (64, 200, 136, 0, True),        # non-negative: exact ties
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_EXACT,
                         ids=lambda c: "x".join(map(str, c[:3]))
                         + ("" if c[3] else "-nonneg"))
def test_gemm_bt_wide_exact(case, monkeypatch):
    M, K, N, lo, rounds = case
    _force(monkeypatch, "wide")
    assert _plan(M, K, N)[0] == "wide"
    A, W, b, ref = _bt_case(M, K, N, lo)
    if rounds:
        rounded, ties = _rounding_stats(ref + b)
        assert rounded > 50 and ties > 20, (rounded, ties)
    _run_bt_exact(A.to(BF16).cuda(), W.to(BF16).cuda(), b, ref,
                  "gemm_bt_wide %s" % ((M, K, N),))


REAL_SHAPES = [(129, 200, 256), (257, 512, 256), (130, 256, 512)]


def _real_case(M, K, N):
    g = torch.Generator().manual_seed(40 + M)
    A = torch.randn(M, K, generator=g).to(BF16)
    W = torch.randn(N, K, generator=g).to(BF16)
    return A, W, torch.randn(N, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", REAL_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_bt_wide_bit_identical_to_narrow(shape, monkeypatch):
    A, W, b = _real_case(*shape)
    A_dev, W_dev, b_dev = A.cuda(), W.cuda(), b.cuda()
    outs = {}
    for which in ("narrow", "wide"):
        _force(monkeypatch, which)
        assert _plan(*shape)[0] == which
        outs[which] = [_C.gemm_bt_bf16(A_dev, W_dev, bias, relu, out_fp32)
                       for bias in (b_dev, None)
                       for relu, out_fp32 in COMBOS]
    for x, y in zip(outs["narrow"], outs["wide"]):
        assert x.dtype == y.dtype and torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", REAL_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_bt_wide_bound(shape, monkeypatch):
    _force(monkeypatch, "wide")
    assert _plan(*shape)[0] == "wide"
    M, K, N = shape
    A, W, b = _real_case(*shape)
    for bias in (b, None):
        bd = torch.zeros(N) if bias is None else bias
        pre = A.double() @ W.double().t() + bd.double()
        mag = A.double().abs() @ W.double().abs().t() + bd.double().abs()
        for relu, out_fp32 in COMBOS:
            ref = pre.clamp(min=0) if relu else pre
            C = _C.gemm_bt_bf16(A.cuda(), W.cuda(),
                                None if bias is None else bias.cuda(),
                                relu, out_fp32)
            _assert_bounded(C, ref, _bound(mag, ref, K, not out_fp32),
                            "gemm_bt_wide %s bias=%s relu=%s fp32=%s" % (
                                shape, bias is not None, relu, out_fp32))


@pytest.mark.gpu
def test_gemm_bt_wide_exact_strided_inputs(monkeypatch):
    """A as a column slice of a wider tensor, Bt as a transposed view: the
    launcher makes contiguous copies, which are 16-byte aligned, so the
    plan stays `wide` and the kernel never sees a stride."""
    _force(monkeypatch, "wide")
    M, K, N = 67, 72, 130
    g = torch.Generator().manual_seed(8)
    wide, Wt, b = _ints((M, K + 13), g), _ints((K, N), g), _ints((N,), g,
                                                                 -8, 8)
    A_dev = wide.to(BF16).cuda()[:, 5:5 + K]
    W_dev = Wt.to(BF16).cuda().t()
    assert not A_dev.is_contiguous() and not W_dev.is_contiguous()
    assert _plan(M, K, N)[0] == "wide"
    _run_bt_exact(A_dev, W_dev, b, wide[:, 5:5 + K] @ Wt,
                  "gemm_bt_wide strided")


@pytest.mark.gpu
def test_gemm_bt_unaligned_base_runs_narrow(monkeypatch):
    """A contiguous A whose first element is 2 bytes past a 16-byte
    boundary is not copied; the launcher plans with aligned=False, which
    is `narrow`, and the result is still exact."""
    _force(monkeypatch, "wide")
    M, K, N = 67, 72, 130
    A, W, b, ref = _bt_case(M, K, N, -3)
    buf = torch.zeros(M * K + 1, dtype=BF16, device="cuda")
    A_dev = buf[1:].view(M, K)
    A_dev.copy_(A.to(BF16))
    assert A_dev.is_contiguous() and A_dev.data_ptr() % 16 == 2
    assert _plan(M, K, N, aligned=False)[0] == "narrow"
    _run_bt_exact(A_dev, W.to(BF16).cuda(), b, ref, "gemm_bt unaligned")

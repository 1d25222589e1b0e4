"""gemm_kt128: the K-major LDS tile image, its transposed fragment reads,
the register prefetch of the next K step and db from the staged tile.

A. Layout, without a GPU.  `_C.gemm_kt_tile_offset(row, chunk)` is the one
   function the kernel stores and reads through: the byte offset of 16-byte
   chunk `chunk` (columns 8*chunk .. 8*chunk+7) of k row `row` in a
   [64][128] bf16 tile.  The tests rebuild from it where every element
   lies, then form the addresses the kernel's lanes form and check them
   against the LDS rules of the hardware: a transposed 8-byte read needs an
   8-byte-aligned address of 4 contiguous elements of one row and is banked
   by (addr / 4) % 64 over each 32-lane half; a 16-byte store is banked by
   (addr / 4) % 32 over each group of 8 consecutive lanes.

B. Exact arithmetic on the GPU, as in test_gemm_family: integer inputs in
   [-3, 3] are exact in bf16, every product is at most 9 and every partial
   sum an integer far below 2^24, so an fp32-accumulating kernel returns
   the exact product bit for bit whatever its chunking.  The reference is
   an fp64 matmul, exact on these integers (sums far below 2^53).  The
   shapes are the smallest that reach the 128x128 kernel (Kb >= 4096) and
   cover every column-tail residue, every row-start alignment of the
   16-byte global loads, and chunks of 1, 2, 3 and 7 K steps with last
   chunks of 1, 32 and 63 rows.

C. One real-valued case against fp64 with the bound of test_gemm_family:
   gamma_{Kb+5} * (|A|^T @ |B|) for dW and gamma_{Kb+5} * sum|A| for db,
   gamma_n = n*u / (1 - n*u), u = 2^-24 (Higham, Accuracy and Stability,
   section 3.1), computed in fp64 in the test.
"""
import functools

import pytest
import torch

from glt_amd import _C

U = 2.0 ** -24
BF16 = torch.bfloat16
ROWS, CHUNKS, TILE_BYTES = 64, 16, 64 * 128 * 2


# --------------------------------------------------------------------------
# A. the tile image (CPU)
# --------------------------------------------------------------------------
def _off(row, ch):
    return _C.gemm_kt_tile_offset(row, ch)


@functools.lru_cache(maxsize=None)
def _element_at():
    """byte address of an element -> (row, column), from the store side:
    element e of chunk ch of row r is written at off(r, ch) + 2e."""
    at = {}
    for r in range(ROWS):
        for ch in range(CHUNKS):
            for e in range(8):
                at[_off(r, ch) + 2 * e] = (r, 8 * ch + e)
    return at


def _tr_lane_addr(r0, c0, q, p):
    """Address lane 4q+p of a 16-lane group supplies for the 4-row block
    at row r0, first chunk c0 (16 columns = chunks c0, c0+1)."""
    return _off(r0 + q, c0 + (p >> 1)) + 8 * (p & 1)


def _max_per_bank(accesses, n_banks):
    """accesses: (byte address, bytes) of the lanes of one group.  The
    largest number of distinct addresses that touch one bank."""
    banks = {}
    for addr, size in set(accesses):
        for d in range(size // 4):
            banks.setdefault((addr // 4 + d) % n_banks, set()).add(addr)
    return max(len(v) for v in banks.values())


def test_tile_offset_is_a_bijection():
    offs = sorted(_off(r, ch) for r in range(ROWS) for ch in range(CHUNKS))
    assert offs == list(range(0, TILE_BYTES, 16))
    assert len(_element_at()) == ROWS * 128


def test_tile_offset_rejects_out_of_range():
    for row, ch in [(-1, 0), (64, 0), (0, -1), (0, 16)]:
        with pytest.raises(RuntimeError):
            _C.gemm_kt_tile_offset(row, ch)


def test_transposed_read_addresses():
    """Every 4-row x 16-column block, rows aligned at 4 and columns at 16:
    the 16 lane addresses are 8-byte aligned and each points at the 4
    contiguous elements (row r0+q, columns 4p .. 4p+3 of the block)."""
    at = _element_at()
    for r0 in range(0, ROWS, 4):
        for c0 in range(0, CHUNKS, 2):
            for q in range(4):
                for p in range(4):
                    addr = _tr_lane_addr(r0, c0, q, p)
                    assert addr % 8 == 0 and 0 <= addr <= TILE_BYTES - 8
                    got = [at[addr + 2 * e] for e in range(4)]
                    want = [(r0 + q, 8 * c0 + 4 * p + e) for e in range(4)]
                    assert got == want, (r0, c0, q, p)


def test_operand_reads_are_conflict_free():
    """The kernel's fragment reads: for k offset kk in {0, 32} and either
    of the two reads (rows +0..3, +4..7), 16-lane group g reads the block
    at row kk + 8g (+4), all four groups in the same 16 columns.  Banks
    are (addr / 4) % 64 over each 32-lane half; every bank at most once."""
    for c0 in range(0, CHUNKS, 2):          # every fragment of A and of B
        for kk in (0, 32):
            for second in (0, 4):
                for half in (0, 1):
                    acc = [(_tr_lane_addr(kk + 8 * g + second, c0, q, p), 8)
                           for g in (2 * half, 2 * half + 1)
                           for q in range(4) for p in range(4)]
                    assert len(acc) == 32
                    assert _max_per_bank(acc, 64) == 1, (c0, kk, second, half)


def test_staging_writes_are_conflict_free():
    """The 16-byte staging stores: thread tid writes chunk tid & 15 of row
    (tid >> 4) + {0, 32}.  A ds_write_b128 is served in 8 groups of 8
    consecutive lanes, banks (addr / 4) % 32, 4 banks per lane: the degree
    of this layout is 1 (every group covers the 32 banks exactly once),
    against 16 for the transposing b32 writes it replaces."""
    worst = 0
    for wave in range(8):
        for h in (0, 32):
            for grp in range(8):
                acc = []
                for lane in range(8 * grp, 8 * grp + 8):
                    tid = 64 * wave + lane
                    acc.append((_off((tid >> 4) + h, tid & 15), 16))
                worst = max(worst, _max_per_bank(acc, 32))
    assert worst == 1


def test_old_layout_degree_by_the_same_rule():
    """The rule of the write test gives 16 for the layout this replaces
    (b32 writes to As[t_c + e][t_k], 72-element rows), so 1 is below it."""
    acc = [(2 * (((tid & 15) * 8) * 72 + (tid >> 4) * 2), 4)
           for tid in range(32)]
    assert _max_per_bank(acc, 32) == 16


def test_db_reads_see_every_row_of_a_column():
    """db reads element (row, column) at off(row, column >> 3) + 2 *
    (column & 7): the store side's address of that element."""
    at = _element_at()
    for r in range(ROWS):
        for m in range(128):
            assert at[_off(r, m >> 3) + 2 * (m & 7)] == (r, m)


# --------------------------------------------------------------------------
# B. exact arithmetic on the GPU
# --------------------------------------------------------------------------
def _mismatch(got, want):
    got = got.detach().cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return "got %s %s, want %s %s" % (got.dtype, tuple(got.shape),
                                          want.dtype, tuple(want.shape))
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    idx = tuple(bad[0].tolist())
    return "%d of %d differ, first at %s: got %r, want %r" % (
        bad.size(0), want.numel(), idx, got[idx].item(), want[idx].item())


def _assert_exact(got, want, what):
    msg = _mismatch(got, want)
    assert msg is None, "%s: %s" % (what, msg)


def _exact_ref(A, B):
    """Integer-valued A, B (any dtype) -> exact fp32 dW and db."""
    Ad, Bd = A.double(), B.double()
    dW, db = Ad.t() @ Bd, Ad.sum(0)
    assert dW.abs().max() < 2 ** 24 and db.abs().max() < 2 ** 24
    return dW.to(torch.float32), db.to(torch.float32)


@functools.lru_cache(maxsize=None)
def _random_case(Kb, M, N):
    g = torch.Generator().manual_seed(5 * Kb + 7 * M + 13 * N)
    A = torch.randint(-3, 4, (Kb, M), generator=g)
    B = torch.randint(-3, 4, (Kb, N), generator=g)
    return (A.to(BF16), B.to(BF16)) + _exact_ref(A, B)


@functools.lru_cache(maxsize=None)
def _position_case(Kb, M, N):
    k = torch.arange(Kb).unsqueeze(1)
    A = (131 * k + 7 * torch.arange(M)) % 5 - 2
    B = (17 * k + 3 * torch.arange(N)) % 7 - 3
    return (A.to(BF16), B.to(BF16)) + _exact_ref(A, B)


def _steps(shape):
    """(K steps per chunk, rows in the last chunk), 128x128 path asserted."""
    big, z, k_per_z = _C.gemm_kt_bf16_plan(*shape)
    assert big, shape
    return k_per_z // 64, shape[0] - (z - 1) * k_per_z


def _run_exact(A, B, dW, db, what):
    """with db, without db (bit-equal dW), and a second call (bit-equal)."""
    A_dev, B_dev = A.cuda(), B.cuda()
    C, d = _C.gemm_kt_bf16(A_dev, B_dev, True)
    _assert_exact(C, dW, "%s dW" % what)
    _assert_exact(d, db, "%s db" % what)
    C2, none = _C.gemm_kt_bf16(A_dev, B_dev, False)
    assert none is None
    assert torch.equal(C2, C), "%s no-db dW: %s" % (what,
                                                    _mismatch(C2, C.cpu()))
    return C, d


TAIL_SHAPES = ([(4096, M, 96) for M in range(128, 137)] +
               [(4096, 128, N) for N in (97, 100, 127, 128, 129, 200, 256)])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TAIL_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_kt128_exact_tails(shape):
    """Every column-tail residue of M (and so every alignment of the row
    starts of A), and N below, at and above the tile and chunk edges."""
    assert _steps(shape) == (1, 64)
    _run_exact(*_random_case(*shape), "gemm_kt128 %s" % (shape,))


# shape, K steps per chunk (None: at least 3), rows in the last chunk
STEP_SHAPES = [
    ((4097, 128, 128), 1, 1),
    ((4159, 128, 128), 1, 63),
    ((12345, 250, 203), 2, 57),
    ((20000, 256, 200), 3, 32),
    ((70000, 128, 128), None, None),
    ((50000, 256, 200), 7, 272),
]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,steps,last", STEP_SHAPES,
                         ids=["x".join(map(str, s[0])) for s in STEP_SHAPES])
def test_gemm_kt128_exact_k_steps(shape, steps, last):
    """Prologue and epilogue of the prefetch: 1, 2, 3 and 7 K steps per
    chunk, last chunks of 1, 32 and 63 rows and of several steps."""
    got_steps, got_last = _steps(shape)
    if steps is None:
        assert got_steps >= 3
    else:
        assert (got_steps, got_last) == (steps, last)
    if shape == (20000, 256, 200):
        assert _C.gemm_kt_bf16_plan(*shape) == (True, 105, 192)
    _run_exact(*_random_case(*shape), "gemm_kt128 %s" % (shape,))


@pytest.mark.gpu
def test_gemm_kt128_exact_position_coded():
    """Inputs that encode (k, m) and (k, n): an A fragment and a B fragment
    that disagree on the order of k are wrong in every output element."""
    shape = (20000, 256, 200)
    assert _steps(shape) == (3, 32)
    A, B, dW, db = _position_case(*shape)
    assert (dW != 0).double().mean() > 0.9      # the check sees every cell
    _run_exact(A, B, dW, db, "gemm_kt128 position-coded")


@pytest.mark.gpu
def test_gemm_kt128_repeatable():
    shape = (20000, 256, 200)
    A, B, dW, db = _random_case(*shape)
    A_dev, B_dev = A.cuda(), B.cuda()
    C1, d1 = _C.gemm_kt_bf16(A_dev, B_dev, True)
    C2, d2 = _C.gemm_kt_bf16(A_dev, B_dev, True)
    assert torch.equal(C1, C2) and torch.equal(d1, d2)
    _assert_exact(C1, dW, "dW")
    _assert_exact(d1, db, "db")


@pytest.mark.gpu
def test_gemm_kt128_exact_strided_A():
    """A as a column slice of a wider tensor (odd width, odd start)."""
    Kb, M, N = 4133, 131, 100
    assert _steps((Kb, M, N))[0] == 1
    g = torch.Generator().manual_seed(9)
    wide = torch.randint(-3, 4, (Kb, M + 19), generator=g)
    B = torch.randint(-3, 4, (Kb, N), generator=g)
    A_dev = wide.to(BF16).cuda()[:, 7:7 + M]
    assert not A_dev.is_contiguous()
    dW, db = _exact_ref(wide[:, 7:7 + M], B)
    C, d = _C.gemm_kt_bf16(A_dev, B.to(BF16).cuda(), True)
    _assert_exact(C, dW, "strided dW")
    _assert_exact(d, db, "strided db")


# --------------------------------------------------------------------------
# C. a derived bound on real-valued inputs
# --------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1.0 - n * U)


def _ratio(got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")),
                                torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return r.max().item()


@pytest.mark.gpu
def test_gemm_kt128_bound():
    Kb, M, N = 20000, 256, 200
    assert _steps((Kb, M, N)) == (3, 32)
    g = torch.Generator().manual_seed(31)
    A = torch.randn(Kb, M, generator=g).to(BF16)
    B = torch.randn(Kb, N, generator=g).to(BF16)
    Ad, Bd = A.double(), B.double()
    C, db = _C.gemm_kt_bf16(A.cuda(), B.cuda(), True)
    r_dw = _ratio(C, Ad.t() @ Bd, _gamma(Kb + 5) * (Ad.abs().t() @ Bd.abs()))
    r_db = _ratio(db, Ad.sum(0), _gamma(Kb + 5) * Ad.abs().sum(0))
    print("GEMM_BOUND gemm_kt128 staging dW %.3g db %.3g" % (r_dw, r_db))
    assert r_dw <= 1.0 and r_db <= 1.0

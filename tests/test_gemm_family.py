"""The MFMA GEMM family: gemm_bt / gemm_bt_persist / gemm_kt / gemm_kt128
(bf16 in, fp32 accumulate) and the fp32 64x64 / 128x128 sage_gemm tiles,
plus the autograd wrappers cast_linear and mfma_linear that reach them.

A. Exact arithmetic.  Inputs are integers in [-3, 3] (biases integers in
   [-8, 8]): exact in bf16 and fp32, every product at most 9, every partial
   sum in any order an integer far below 2^24.  An fp32-accumulating kernel
   must therefore return the int64 matmul bit for bit, whatever its tiling,
   split-K plan or summation order; a bf16 output must be that integer
   rounded once to nearest-even, `ref.float().to(bfloat16)`.  Integers up
   to 256 are exact in bf16, and a sum of K products of two uniform [-3, 3]
   draws has standard deviation 4*sqrt(K), so the rounding is only
   exercised by K = 2000 (sigma 179) and by a non-negative variant (inputs
   in [0, 3], mean product 2.25: sums near 450 at K = 200, where odd
   integers are exact ties).  Those cases assert that they do round.

B. Derived bounds on real-valued inputs.  u = 2^-24, gamma_n = n*u/(1-n*u).
   Inputs are randn cast to the kernel's input dtype and then taken to
   fp64, so the reference sees exactly what the kernel sees.  For any
   order of an fp32 dot product of length K plus a bias add
       e32 = gamma_{K+5} * (|A| @ |B| + |bias|)          (elementwise)
   bounds the error (Higham, Accuracy and Stability, section 3.1; the +5
   leaves room for the product roundings, the bias add and the split-K
   fold, which is one more fp32 sum over the same terms).  db, a plain
   column sum, gets gamma_{Kb+5} * sum|A|.  ReLU is 1-Lipschitz, so e32
   holds after it with ref = relu(ref).  A bf16 output is the fp32 value
   rounded once to nearest-even: off by at most half a bf16 ulp of a value
   that is at most x = |ref| + e32.  bf16 keeps 8 significant bits, so
   with 2^(e-1) <= x < 2^e the ulp is 2^(e-8) and
       ebf = 2^(e-9) + e32
   which lies between 2^-9 * x and 2^-8 * x (2^-8 is the unit roundoff of
   the format; a flat 2^-9 * x would reject a correctly rounded result in
   the lower part of every binade).  Truncation instead of rounding errs
   by up to a whole ulp and fails this bound.  The bounds are computed in
   fp64 inside the tests; nothing is fitted to the kernels' output.  Each
   test prints max(err / bound), which must be <= 1.

C. CPU self-checks (unmarked): torch emulations of five plausible kernel
   defects must be rejected by the checks of A and B, and a correct
   fp32-accumulate emulation must pass them.
"""
import functools

import pytest
import torch

from glt_amd import _C

U = 2.0 ** -24
BF16 = torch.bfloat16
COMBOS = [(relu, out_fp32) for relu in (False, True)
          for out_fp32 in (False, True)]


# --------------------------------------------------------------------------
# the two checks
# --------------------------------------------------------------------------
def _mismatch(got, want):
    """None when `got` is bit-for-bit `want`, else a description of the
    first differing element."""
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


def _gamma(n):
    return n * U / (1.0 - n * U)


def _bound(mag, ref, k, bf16_out):
    """mag = |A| @ |B| + |bias| (fp64), ref fp64, k the reduction length."""
    e32 = _gamma(k + 5) * mag
    if not bf16_out:
        return e32
    return _half_ulp_bf16(ref.abs() + e32) + e32


def _half_ulp_bf16(x):
    """Half the spacing of bf16 (8 significant bits) at x >= 0, fp64."""
    _, e = torch.frexp(x)              # x = m * 2^e, 0.5 <= m < 1
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9),
                       torch.zeros_like(x))


def _ratio(got, ref, bound):
    """max(err / bound); an error where the bound is 0 counts as inf."""
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")),
                                torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return r.max().item() if r.numel() else 0.0


def _assert_bounded(got, ref, bound, what):
    r = _ratio(got, ref, bound)
    print("GEMM_BOUND %s: max err/bound %.3g" % (what, r))
    assert r <= 1.0, "%s: max err/bound %.3g" % (what, r)


def _ints(shape, gen, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen)


def _to_bf16_rne(v):
    """int64 -> the bf16 a single round-to-nearest-even gives."""
    return v.to(torch.float32).to(BF16)


def _rounding_stats(v):
    """(# values a bf16 cannot hold, # of those that are exact ties)."""
    d = (v - _to_bf16_rne(v).to(torch.float64).to(torch.int64)).abs()
    e = torch.floor(torch.log2(v.abs().clamp(min=1).double()))
    spacing = 2.0 ** (e - 7)
    return int((d > 0).sum()), int(((d > 0) & (d.double() * 2 == spacing))
                                   .sum())


# --------------------------------------------------------------------------
# C. CPU self-checks: the checks above have teeth
# --------------------------------------------------------------------------
def _trunc_bf16(x):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    bits = x.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF16)


def _emu_bt(A, W, bias, mode="ok", out_bf16=True):
    """Torch emulation of C = A @ W^T + bias, correct or with one defect."""
    A, W = A.float(), W.float()
    bias = None if bias is None else bias.float()
    if mode == "drop_elem":        # last k of the last row never staged
        A = A.clone()
        A[-1, -1] = 0
    if mode == "no_bias_last":     # epilogue skips the last column's bias
        bias = bias.clone()
        bias[-1] = 0
    if mode == "step64":           # accumulator kept in bf16 between steps
        acc = torch.zeros(A.size(0), W.size(0))
        for k0 in range(0, A.size(1), 64):
            acc = (acc + A[:, k0:k0 + 64] @ W[:, k0:k0 + 64].t()
                   ).to(BF16).float()
    else:
        acc = A @ W.t()
    if bias is not None:
        acc = acc + bias
    if not out_bf16:
        return acc
    return _trunc_bf16(acc) if mode == "trunc" else acc.to(BF16)


def _emu_kt(A, B, mode="ok"):
    if mode == "drop_row":         # second row of the last pair not loaded
        A, B = A[:-1], B[:-1]
    return A.float().t() @ B.float()


def _selfcheck_int_case():
    g = torch.Generator().manual_seed(100)
    M, K, N = 67, 2000, 70
    A, W, b = _ints((M, K), g), _ints((N, K), g), _ints((N,), g, -8, 8)
    A[-1, -1] = 3                  # make the two planted defects visible
    W[:, -1] = torch.where(W[:, -1] == 0, 1, W[:, -1])
    b[-1] = 5
    return A, W, b, A @ W.t() + b


def _selfcheck_real_case():
    g = torch.Generator().manual_seed(101)
    M, K, N = 130, 200, 70
    A = torch.randn(M, K, generator=g).to(BF16)
    W = torch.randn(N, K, generator=g).to(BF16)
    b = torch.randn(N, generator=g)
    ref = A.double() @ W.double().t() + b.double()
    mag = A.double().abs() @ W.double().abs().t() + b.double().abs()
    return A, W, b, ref, mag, K


@pytest.mark.parametrize("mode", ["trunc", "step64", "drop_elem",
                                  "no_bias_last"])
def test_selfcheck_exact_rejects_bt_defects(mode):
    A, W, b, ref = _selfcheck_int_case()
    want = _to_bf16_rne(ref)
    assert _mismatch(_emu_bt(A, W, b), want) is None
    assert _mismatch(_emu_bt(A, W, b, out_bf16=False),
                     ref.to(torch.float32)) is None
    msg = _mismatch(_emu_bt(A, W, b, mode), want)
    assert msg is not None and "first at" in msg


def test_selfcheck_exact_rejects_dropped_odd_row():
    g = torch.Generator().manual_seed(102)
    Kb, M, N = 131, 40, 30
    A, B = _ints((Kb, M), g), _ints((Kb, N), g)
    want = (A.t() @ B).to(torch.float32)
    assert _mismatch(_emu_kt(A, B), want) is None
    assert _mismatch(_emu_kt(A, B, "drop_row"), want) is not None


@pytest.mark.parametrize("mode", ["trunc", "step64"])
def test_selfcheck_bound_rejects_precision_defects(mode):
    A, W, b, ref, mag, K = _selfcheck_real_case()
    bound = _bound(mag, ref, K, True)
    assert _ratio(_emu_bt(A, W, b, mode), ref, bound) > 1.0


def test_selfcheck_bound_accepts_fp32_accumulate():
    A, W, b, ref, mag, K = _selfcheck_real_case()
    assert _ratio(_emu_bt(A, W, b), ref, _bound(mag, ref, K, True)) <= 1.0
    assert _ratio(_emu_bt(A, W, b, out_bf16=False), ref,
                  _bound(mag, ref, K, False)) <= 1.0
    # and the bound check is not vacuous where the bound is zero
    z = torch.zeros(2, 2, dtype=torch.float64)
    assert _ratio(torch.ones(2, 2), z, z) == float("inf")
    assert _ratio(torch.zeros(2, 2), z, z) == 0.0


def test_selfcheck_rounding_is_exercised():
    """The cases that pin round-to-nearest-even do produce values that
    bf16 cannot hold, exact ties among them."""
    for key in [(70, 2000, 70, -3), (64, 200, 70, 0)]:
        A, W, b, ref = _bt_case(*key)
        rounded, ties = _rounding_stats(ref + b)
        assert rounded > 50 and ties > 20, (key, rounded, ties)


# --------------------------------------------------------------------------
# gemm_kt plan (host arithmetic: checked with and without a GPU)
# --------------------------------------------------------------------------
# (Kb, M, N), big, z, k_per_z, rows in the last chunk; None = not pinned
KT_PLAN = [
    ((1, 40, 30), False, 1, 64, 1),            # one row
    ((63, 64, 64), False, 1, 64, 63),          # odd tail
    ((131, 40, 30), False, 3, 64, 3),          # last chunk 3 rows
    ((9001, 509, 77), False, 47, 192, 169),    # 3 K steps/chunk, odd M, N
    ((4133, 131, 100), True, 65, 64, 37),      # M tail 3, scalar N tail
    ((12345, 250, 203), True, 97, 128, 57),    # 2 K steps/chunk
    ((4096, 128, 96), True, None, None, None),   # the dispatch boundary
    ((4095, 128, 96), False, None, None, None),  # and its three
    ((4096, 127, 96), False, None, None, None),  # neighbours
    ((4096, 128, 95), False, None, None, None),
]
KT_IDS = ["x".join(map(str, p[0])) for p in KT_PLAN]


def _assert_plan(shape, big, z, k_per_z, last):
    got_big, got_z, got_k = _C.gemm_kt_bf16_plan(*shape)
    assert got_big == big, (shape, got_big)
    if z is not None:
        assert (got_z, got_k) == (z, k_per_z), (shape, got_z, got_k)
        assert shape[0] - (got_z - 1) * got_k == last
    # the chunks cover Kb, in whole 64-row K steps, none of them empty
    assert got_k % 64 == 0 and got_k >= 64 and got_z >= 1
    assert (got_z - 1) * got_k < max(shape[0], 1) <= got_z * got_k


@pytest.mark.parametrize("plan", KT_PLAN, ids=KT_IDS)
def test_gemm_kt_plan_table(plan):
    _assert_plan(*plan)


def test_gemm_kt_plan_degenerate_sizes():
    """Zero sizes divide by nothing and plan one chunk row range."""
    for shape in [(0, 5, 5), (200, 0, 5), (200, 5, 0), (0, 0, 0),
                  (5000, 0, 0)]:
        _assert_plan(shape, False, None, None, None)


# --------------------------------------------------------------------------
# A. exact arithmetic on the GPU
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bt_case(M, K, N, lo):
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N)
    A, W = _ints((M, K), g, lo), _ints((N, K), g, lo)
    return A, W, _ints((N,), g, -8, 8), A @ W.t()


def _bt_want(ref, b, relu, out_fp32):
    v = ref if b is None else ref + b
    if relu:
        v = v.clamp(min=0)
    return v.to(torch.float32) if out_fp32 else _to_bf16_rne(v)


def _run_bt_exact(A_dev, W_dev, b, ref, what):
    """All (relu, out_fp32) x (bias, no bias) against the int64 result;
    returns the outputs for a bit comparison between kernels."""
    outs = []
    for bias in (b, None):
        bias_dev = None if bias is None else bias.float().cuda()
        for relu, out_fp32 in COMBOS:
            C = _C.gemm_bt_bf16(A_dev, W_dev, bias_dev, relu, out_fp32)
            _assert_exact(C, _bt_want(ref, bias, relu, out_fp32),
                          "%s bias=%s relu=%s fp32=%s" % (
                              what, bias is not None, relu, out_fp32))
            outs.append(C)
    return outs


# (M, K, N, lowest input value): lo = 0 is the non-negative variant
BT_SHAPES = [(1, 1, 1), (4, 7, 64), (63, 15, 47), (65, 16, 65),
             (64, 17, 64), (130, 31, 129), (33, 33, 33), (64, 63, 64),
             (64, 64, 64), (67, 65, 70), (130, 100, 47), (257, 129, 200),
             (5, 0, 70)]
BT_SHAPES = [s + (-3,) for s in BT_SHAPES] + [(64, 200, 70, 0)]
BT_DEFAULT_ONLY = [(70, 2000, 70, -3)]   # K > 256: no persistent form


def _bt_id(s):
    return "x".join(map(str, s[:3])) + ("" if s[3] else "-nonneg")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BT_SHAPES + BT_DEFAULT_ONLY, ids=_bt_id)
def test_gemm_bt_exact(shape, monkeypatch):
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    A, W, b, ref = _bt_case(*shape)
    _run_bt_exact(A.to(BF16).cuda(), W.to(BF16).cuda(), b, ref,
                  "gemm_bt %s" % (shape,))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BT_SHAPES + [(66000, 40, 64, -3)],
                         ids=_bt_id)
def test_gemm_bt_persist_exact(shape, monkeypatch):
    """The persistent-B kernel (K <= 256), bit-equal to the int64 result
    and to the default kernel.  66000 rows are 1032 m-tiles over a grid
    capped at 1024, so the m-tile stride loop wraps."""
    assert shape[1] <= 256
    A, W, b, ref = _bt_case(*shape)
    A_dev, W_dev = A.to(BF16).cuda(), W.to(BF16).cuda()
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    base = _run_bt_exact(A_dev, W_dev, b, ref, "gemm_bt %s" % (shape,))
    monkeypatch.setenv("GLT_GEMM_PERSIST", "1")
    pers = _run_bt_exact(A_dev, W_dev, b, ref,
                         "gemm_bt_persist %s" % (shape,))
    for x, y in zip(base, pers):
        assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("persist", [False, True])
def test_gemm_bt_exact_strided_inputs(persist, monkeypatch):
    """A as a column slice of a wider tensor, Bt as a transposed view."""
    if persist:
        monkeypatch.setenv("GLT_GEMM_PERSIST", "1")
    else:
        monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    M, K, N = 67, 65, 70
    g = torch.Generator().manual_seed(7)
    wide, Wt, b = _ints((M, K + 13), g), _ints((K, N), g), _ints((N,), g,
                                                                 -8, 8)
    A_dev = wide.to(BF16).cuda()[:, 5:5 + K]
    W_dev = Wt.to(BF16).cuda().t()
    assert not A_dev.is_contiguous() and not W_dev.is_contiguous()
    _run_bt_exact(A_dev, W_dev, b, wide[:, 5:5 + K] @ Wt, "gemm_bt strided")


@pytest.mark.gpu
@pytest.mark.parametrize("persist", [False, True])
def test_gemm_bt_zero_sizes(persist, monkeypatch):
    if persist:
        monkeypatch.setenv("GLT_GEMM_PERSIST", "1")
    else:
        monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    for M, K, N in [(5, 16, 0), (0, 16, 5), (0, 0, 0), (5, 0, 0)]:
        A = torch.zeros(M, K, dtype=BF16, device="cuda")
        W = torch.zeros(N, K, dtype=BF16, device="cuda")
        b = torch.zeros(N, device="cuda")
        for relu, out_fp32 in COMBOS:
            C = _C.gemm_bt_bf16(A, W, b, relu, out_fp32)
            assert C.shape == (M, N)
            assert C.dtype == (torch.float32 if out_fp32 else BF16)
    _assert_no_pending_error()


def _assert_no_pending_error():
    """A failed launch stays behind as the runtime's last error until the
    next launch check reads it: launch something and synchronize."""
    torch.cuda.synchronize()
    assert torch.zeros(3, device="cuda").add_(1).sum().item() == 3.0
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _kt_case(Kb, M, N):
    g = torch.Generator().manual_seed(Kb + 7 * M + 13 * N)
    A, B = _ints((Kb, M), g), _ints((Kb, N), g)
    return A, B, (A.t() @ B).to(torch.float32), A.sum(0).to(torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", KT_PLAN, ids=KT_IDS)
def test_gemm_kt_exact(plan):
    shape = plan[0]
    _assert_plan(*plan)
    A, B, ref, dbref = _kt_case(*shape)
    A_dev, B_dev = A.to(BF16).cuda(), B.to(BF16).cuda()
    C, db = _C.gemm_kt_bf16(A_dev, B_dev, True)
    _assert_exact(C, ref, "gemm_kt dW %s" % (shape,))
    _assert_exact(db, dbref, "gemm_kt db %s" % (shape,))
    C2, none = _C.gemm_kt_bf16(A_dev, B_dev, False)
    assert none is None
    assert torch.equal(C2, C), _mismatch(C2, C.cpu())


@pytest.mark.gpu
def test_gemm_kt_zero_sizes():
    g = torch.Generator().manual_seed(3)
    for Kb, M, N in [(0, 70, 33), (200, 0, 33), (200, 70, 0), (0, 0, 0)]:
        A, B = _ints((Kb, M), g), _ints((Kb, N), g)
        A_dev, B_dev = A.to(BF16).cuda(), B.to(BF16).cuda()
        C, db = _C.gemm_kt_bf16(A_dev, B_dev, True)
        _assert_exact(C, torch.zeros(M, N), "dW %s" % ((Kb, M, N),))
        # db = colsum(A) does not depend on N: zeros only when Kb == 0
        _assert_exact(db, A.sum(0).to(torch.float32),
                      "db %s" % ((Kb, M, N),))
        C2, none = _C.gemm_kt_bf16(A_dev, B_dev, False)
        assert none is None
        _assert_exact(C2, torch.zeros(M, N), "dW %s" % ((Kb, M, N),))
    _assert_no_pending_error()


SAGE_SHAPES = [(1, 1, 64), (65, 17, 128), (130, 100, 64), (127, 400, 128),
               (128, 384, 128), (129, 385, 128), (200, 415, 256),
               (333, 513, 128)]


def _sage_is_128(M, K, N):
    return N % 128 == 0 and M >= 128 and K >= 384


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SAGE_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_sage_gemm_exact(shape):
    M, K, N = shape
    g = torch.Generator().manual_seed(M + K + N)
    A, B, b = _ints((M, K), g), _ints((K, N), g), _ints((N,), g, -8, 8)
    ref = A @ B
    A_dev, B_dev = A.float().cuda(), B.float().cuda()
    for bias in (b, None):
        bias_dev = None if bias is None else bias.float().cuda()
        for relu in (False, True):
            want = ref if bias is None else ref + bias
            want = want.clamp(min=0) if relu else want
            _assert_exact(_C.sage_gemm(A_dev, B_dev, bias_dev, relu),
                          want.to(torch.float32),
                          "sage_gemm %s bias=%s relu=%s" % (
                              shape, bias is not None, relu))


@pytest.mark.gpu
def test_sage_gemm_zero_sizes():
    for M, K, N in [(5, 16, 0), (0, 16, 64), (0, 0, 0)]:
        A = torch.zeros(M, K, device="cuda")
        B = torch.zeros(K, N, device="cuda")
        for relu in (False, True):
            C = _C.sage_gemm(A, B, torch.zeros(N, device="cuda"), relu)
            assert C.shape == (M, N) and C.dtype == torch.float32
    _assert_no_pending_error()


# --- autograd wrappers ------------------------------------------------------
def _linear_int_case(batch, fin, fout, relu, seed):
    """Integer x, W, b, dy and the int64 forward / dx / dW / db.  Integer
    pre-activations make the ReLU mask the same in kernel and reference."""
    g = torch.Generator().manual_seed(seed)
    x, w = _ints((batch, fin), g), _ints((fout, fin), g)
    b, dy = _ints((fout,), g, -8, 8), _ints((batch, fout), g)
    out = x @ w.t() + b
    if relu:
        dyr = dy * (out > 0)
        out = out.clamp(min=0)
        assert 0.2 < (dyr != dy).double().mean() < 0.8  # the mask matters
    else:
        dyr = dy
    return x, w, b, dy, out, dyr @ w, dyr.t() @ x, dyr.sum(0), dyr


# (batch, in, out, gemm_kt reaches the 128x128 kernel)
CAST_SHAPES = [(300, 64, 64, False), (4200, 128, 128, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", CAST_SHAPES,
                         ids=lambda s: "x".join(map(str, s[:3])))
def test_cast_linear_exact(shape, relu, monkeypatch):
    from glt_amd.ops import cast_linear

    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    monkeypatch.delenv("GLT_DISABLE_BF16_MFMA", raising=False)
    batch, fin, fout, big = shape
    assert fin % 16 == 0 and fout >= 32        # dx and all on the kernels
    assert _C.gemm_kt_bf16_plan(batch, fout, fin)[0] == big
    x, w, b, dy, out, dx, dw, db, _ = _linear_int_case(batch, fin, fout,
                                                       relu, 11)
    xd = x.to(BF16).cuda().requires_grad_(True)
    wd = w.float().cuda().requires_grad_(True)
    bd = b.float().cuda().requires_grad_(True)
    y = cast_linear(xd, wd, bd, relu=relu)
    y.backward(dy.to(BF16).cuda())
    _assert_exact(y, _to_bf16_rne(out), "forward")
    _assert_exact(xd.grad, _to_bf16_rne(dx), "dx")
    _assert_exact(wd.grad, dw.to(torch.float32), "dW")
    _assert_exact(bd.grad, db.to(torch.float32), "db")


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
def test_cast_linear_library_dx(relu, monkeypatch):
    """in-features = 100: forward, dW and db stay on the kernels (exact);
    dx is the library's bf16 GEMM, held to the bf16 bound of section B."""
    from glt_amd.ops import cast_linear

    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    monkeypatch.delenv("GLT_DISABLE_BF16_MFMA", raising=False)
    batch, fin, fout = 300, 100, 64
    x, w, b, dy, out, dx, dw, db, dyr = _linear_int_case(batch, fin, fout,
                                                         relu, 12)
    xd = x.to(BF16).cuda().requires_grad_(True)
    wd = w.float().cuda().requires_grad_(True)
    bd = b.float().cuda().requires_grad_(True)
    y = cast_linear(xd, wd, bd, relu=relu)
    y.backward(dy.to(BF16).cuda())
    _assert_exact(y, _to_bf16_rne(out), "forward")
    _assert_exact(wd.grad, dw.to(torch.float32), "dW")
    _assert_exact(bd.grad, db.to(torch.float32), "db")
    mag = dyr.abs().double() @ w.abs().double()
    _assert_bounded(xd.grad, dx.double(), _bound(mag, dx.double(), fout,
                                                 True),
                    "cast_linear library dx relu=%s" % relu)


# (batch, in, out): the 64x64 and the 128x128 forward kernel
MFMA_SHAPES = [(130, 64, 64), (200, 448, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", MFMA_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_mfma_linear_exact(shape, relu):
    from glt_amd.ops import mfma_linear

    batch, fin, fout = shape
    assert fin % 64 == 0 and fout % 64 == 0    # dx on the kernel too
    x, w, b, dy, out, dx, dw, db, _ = _linear_int_case(batch, fin, fout,
                                                       relu, 13)
    xd = x.float().cuda().requires_grad_(True)
    wd = w.float().cuda().requires_grad_(True)
    bd = b.float().cuda().requires_grad_(True)
    y = mfma_linear(xd, wd, bd, relu=relu)
    y.backward(dy.float().cuda())
    _assert_exact(y, out.to(torch.float32), "forward")
    _assert_exact(xd.grad, dx.to(torch.float32), "dx")
    _assert_exact(wd.grad, dw.to(torch.float32), "dW")
    _assert_exact(bd.grad, db.to(torch.float32), "db")


# --------------------------------------------------------------------------
# B. derived bounds on real-valued inputs
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("persist", [False, True],
                         ids=["gemm_bt", "gemm_bt_persist"])
@pytest.mark.parametrize("shape", [(63, 15, 47), (257, 129, 200)],
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_bt_bound(shape, persist, monkeypatch):
    if persist:
        monkeypatch.setenv("GLT_GEMM_PERSIST", "1")
    else:
        monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    M, K, N = shape
    g = torch.Generator().manual_seed(20 + M)
    A = torch.randn(M, K, generator=g).to(BF16)
    W = torch.randn(N, K, generator=g).to(BF16)
    b = torch.randn(N, generator=g)
    pre = A.double() @ W.double().t() + b.double()
    mag = A.double().abs() @ W.double().abs().t() + b.double().abs()
    name = "gemm_bt_persist" if persist else "gemm_bt"
    for relu, out_fp32 in COMBOS:
        ref = pre.clamp(min=0) if relu else pre
        C = _C.gemm_bt_bf16(A.cuda(), W.cuda(), b.cuda(), relu, out_fp32)
        _assert_bounded(C, ref, _bound(mag, ref, K, not out_fp32),
                        "%s %s relu=%s fp32=%s" % (name, shape, relu,
                                                   out_fp32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,big", [
    ((131, 40, 30), False), ((9001, 509, 77), False),
    ((4133, 131, 100), True), ((12345, 250, 203), True)],
    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_gemm_kt_bound(shape, big):
    Kb, M, N = shape
    assert _C.gemm_kt_bf16_plan(Kb, M, N)[0] == big
    g = torch.Generator().manual_seed(30 + M)
    A = torch.randn(Kb, M, generator=g).to(BF16)
    B = torch.randn(Kb, N, generator=g).to(BF16)
    ref = A.double().t() @ B.double()
    mag = A.double().abs().t() @ B.double().abs()
    C, db = _C.gemm_kt_bf16(A.cuda(), B.cuda(), True)
    name = "gemm_kt128" if big else "gemm_kt"
    _assert_bounded(C, ref, _bound(mag, ref, Kb, False),
                    "%s dW %s" % (name, shape))
    _assert_bounded(db, A.double().sum(0),
                    _gamma(Kb + 5) * A.double().abs().sum(0),
                    "%s db %s" % (name, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(65, 17, 128), (127, 400, 128),
                                   (129, 385, 128), (333, 513, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_sage_gemm_bound(shape):
    M, K, N = shape
    g = torch.Generator().manual_seed(40 + M)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(K, N, generator=g)
    b = torch.randn(N, generator=g)
    pre = A.double() @ B.double() + b.double()
    mag = A.double().abs() @ B.double().abs() + b.double().abs()
    name = "sage_gemm_128" if _sage_is_128(M, K, N) else "sage_gemm_64"
    for relu in (False, True):
        ref = pre.clamp(min=0) if relu else pre
        C = _C.sage_gemm(A.cuda(), B.cuda(), b.cuda(), relu)
        _assert_bounded(C, ref, _bound(mag, ref, K, False),
                        "%s %s relu=%s" % (name, shape, relu))

"""Segment-mean kernels (ops.segment_mean / ops.segment_mean_cat), one
case per dispatch branch of csrc/hip/hip_segment.hip.

    mean    : out[t, :]  = mean_{e in seg(t)} x[col[e], :]   (0 if empty)
              dx[c, :]  += dy[t, :] / deg(t)                  per edge (t, c)
    mean_cat: out[t, :F] = the mean, out[t, F:] = x[t, :]
              dx as above from dy[:, :F], plus dx[t, :] += dy[t, F:]

Exact cases.  x and dy are integers in [-4, 4] and every degree is a power
of two <= 32 (or 0).  Each segment sum is then an integer of magnitude
<= 128, 1/deg is a power of two, and each mean is a dyadic rational with
at most 8 significant bits: exact in fp32 and in bf16 in any summation
order.  Each dx term is a multiple of 2^-5 of magnitude <= 4 and a dx row
collects far fewer than 128 of them, so the fp32 arena is exact too and a
bf16 dx is that exact value rounded once.  Forward and backward must
therefore equal the fp64 reference cast to the output dtype bit for bit.
In deterministic mode max|dy| = 4 gives 2^e = 8 and the snap grid
q = 2^(3 + 6 - 24) = 2^-15; every term is a multiple of 2^-5, hence on the
grid (no rounding, no ties), and no dx element comes near the 2^6 * 2^e =
512 headroom (asserted), so both modes must return the same bits.

Mixed-degree cases (3, 9, 12, 17, 24: full batches of 8 and partial
tails).  The sums stay exact; fl(1/deg) and the product round once each:
    forward fp32: |out - ref| <= 2^-22 |ref|  ((1 + 2^-24)^2 - 1 < 2^-22)
    forward bf16: |out - ref| <= 2^-8 |ref|   (one more rounding: half a
                  bf16 ulp, 2^-8 of the binade's lower end)
    dx fp32     : (cnt_c + 2) * 2^-24 * sum|terms|, cnt_c = terms landing
                  on row c: two roundings per term plus cnt_c - 1 fp32
                  additions in any order
    dx bf16     : the fp32 arena rounded once: 2^-8 (|ref| + b32) + b32,
                  the form tests/test_weighted_segment.py uses
All bounds are computed in fp64 inside the tests; none is fitted.

The forward accumulator cannot be caught rounding to bf16 by these inputs
(integers up to 256 are exact in bf16); the long-segment case in
test_gpu.py::test_segment_mean_bf16_numerics holds that.  The dx arena is
caught: 8 + 2^-5 needs nine bits.
"""
import pytest
import torch

from glt_amd import _C

F32, BF16 = torch.float32, torch.bfloat16
EXACT_DEGS = (0, 1, 2, 4, 8, 16, 32)
MIXED_DEGS = (0, 3, 9, 12, 17, 1, 24)
# fp32: one column, two columns, the 128-channel fast-path edge, fallback
# loop; bf16 even F (bf16x2 kernel): feat2 = 64 edge, feat2 = 65 fallback;
# bf16 odd F: the scalar template on bf16, fast path and fallback
SHAPES = [(F32, f) for f in (1, 64, 65, 100, 128, 129, 200)] + \
         [(BF16, f) for f in (2, 100, 128, 130, 256)] + \
         [(BF16, f) for f in (1, 63, 127, 129)]
SHAPE_IDS = ["%s-F%d" % ("fp32" if d == F32 else "bf16", f)
             for d, f in SHAPES]
N_TGT, N_SRC = 37, 50   # 37: not a multiple of the 4 waves per block


# --------------------------------------------------------------------------
# case builder, fp64 reference, fp32 emulation of the kernels
# --------------------------------------------------------------------------
def _case(F, dtype, degs, n_tgt=N_TGT, n_src=N_SRC, seed=0, device="cpu"):
    """Degrees cycle through `degs`; col is random with repeats; x is
    [n_src, F] and dy [n_tgt, 2F] (the plain mean uses its left half)."""
    g = torch.Generator().manual_seed(1000 * seed + F)
    deg = torch.tensor(degs).repeat(n_tgt // len(degs) + 1)[:n_tgt]
    tgt = torch.repeat_interleave(torch.arange(n_tgt), deg)
    col = torch.randint(0, n_src, (tgt.numel(),), generator=g)
    x = torch.randint(-4, 5, (n_src, F), generator=g).to(dtype)
    dy = torch.randint(-4, 5, (n_tgt, 2 * F), generator=g).to(dtype)
    dy[0, 0] = 4    # max|dy| = 4 whatever the draw: the 2^-15 grid
    return dict(x=x.to(device), dy=dy.to(device), tgt=tgt.to(device),
                col=col.to(device), n_tgt=n_tgt, F=F, dtype=dtype)


def _dy(case, cat):
    return case["dy"] if cat else case["dy"][:, :case["F"]].contiguous()


def _reference(case, cat):
    """fp64 (out, dx, sum |dx terms|, number of terms per dx row)."""
    x, dy = case["x"].double(), case["dy"].double()
    tgt, col, n_tgt, F = case["tgt"], case["col"], case["n_tgt"], case["F"]
    off = torch.searchsorted(tgt, torch.arange(n_tgt + 1, device=tgt.device))
    deg = (off[1:] - off[:-1]).double().unsqueeze(1)
    out = torch.zeros(n_tgt, F, dtype=torch.float64, device=x.device)
    out.index_add_(0, tgt, x[col])
    out = out / deg.clamp(min=1)
    terms = dy[tgt, :F] / deg[tgt]
    dx, mag = torch.zeros_like(x), torch.zeros_like(x)
    dx.index_add_(0, col, terms)
    mag.index_add_(0, col, terms.abs())
    cnt = torch.zeros(x.size(0), dtype=torch.float64, device=x.device)
    cnt.index_add_(0, col, torch.ones_like(col, dtype=torch.float64))
    if cat:
        out = torch.cat([out, x[:n_tgt]], dim=1)
        dx[:n_tgt] += dy[:, F:]
        mag[:n_tgt] += dy[:, F:].abs()
        cnt[:n_tgt] += 1
    return out, dx, mag, cnt


def _emulate(case, cat, defect=None):
    """What the kernels compute, edge by edge in fp32 on the CPU, with an
    optional defect.  Returns (out, dx) in the case's dtype."""
    x, dy = case["x"].float(), case["dy"].float()
    tgt, col, n_tgt, F = case["tgt"], case["col"], case["n_tgt"], case["F"]
    off = torch.searchsorted(tgt, torch.arange(n_tgt + 1)).tolist()

    def acc(v):
        return v.to(BF16).float() if defect == "bf16_accumulator" else v

    mean = torch.zeros(n_tgt, F)
    dx = torch.zeros_like(x)
    if cat and defect != "no_root_gradient":
        dx[:n_tgt] = acc(dy[:, F:])
    for t in range(n_tgt):
        s, e = off[t], off[t + 1]
        if e == s:
            continue
        div = e - s + (1 if defect == "deg_plus_one" else 0)
        inv = torch.tensor(1.0) / torch.tensor(float(div))
        if defect == "tail_batch_dropped":
            e = s + (e - s) // 8 * 8
        a = torch.zeros(F)
        for k in range(s, e):
            a = acc(a + x[col[k]])
            dx[col[k]] = acc(dx[col[k]] + dy[t, :F] * inv)
        mean[t] = a * inv
    out = mean
    if cat:
        halves = [mean, x[:n_tgt]]
        out = torch.cat(halves[::-1] if defect == "halves_swapped"
                        else halves, dim=1)
    return out.to(case["dtype"]), dx.to(case["dtype"])


def _exact(got, ref, dtype):
    return got.dtype == dtype and torch.equal(got, ref.to(dtype))


# --------------------------------------------------------------------------
# CPU self-checks
# --------------------------------------------------------------------------
@pytest.mark.parametrize("cat", [False, True])
@pytest.mark.parametrize("degs", [EXACT_DEGS, MIXED_DEGS])
def test_reference_matches_torch_composition(degs, cat):
    """The fp64 builder against the composition SAGEConv falls back to
    (index_add_ / bincount / cat) and its autograd gradient."""
    case = _case(7, torch.float64, degs)
    x = case["x"].clone().requires_grad_(True)
    tgt, col, n_tgt = case["tgt"], case["col"], case["n_tgt"]
    agg = x.new_zeros(n_tgt, 7)
    agg.index_add_(0, tgt, x.index_select(0, col))
    deg = torch.bincount(tgt, minlength=n_tgt).clamp(min=1)
    comp = agg / deg.unsqueeze(1).to(x.dtype)
    if cat:
        comp = torch.cat([comp, x[:n_tgt]], dim=1)
    comp.backward(_dy(case, cat))
    out, dx, _, cnt = _reference(case, cat)
    assert torch.allclose(out, comp.detach(), rtol=1e-14, atol=0)
    assert torch.allclose(dx, x.grad, rtol=1e-13, atol=1e-14)
    assert torch.equal(cnt, torch.bincount(col, minlength=N_SRC).double()
                       + (torch.arange(N_SRC) < n_tgt) * float(cat))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_cases_have_one_answer_and_reject_defects(dtype):
    case = _case(5, dtype, EXACT_DEGS)
    # all edges on three rows: their partial sums pass 8 while they carry
    # 2^-5 fractions, which a bf16 arena cannot hold
    case["col"] %= 3
    for cat in (False, True):
        ref_out, ref_dx, mag, _ = _reference(case, cat)
        assert mag.max().item() < 512
        out, dx = _emulate(case, cat)
        assert _exact(out, ref_out, dtype) and _exact(dx, ref_dx, dtype)
        defects = ["tail_batch_dropped", "deg_plus_one", "bf16_accumulator"]
        if cat:
            defects += ["halves_swapped", "no_root_gradient"]
        for defect in defects:
            out, dx = _emulate(case, cat, defect)
            assert not (_exact(out, ref_out, dtype)
                        and _exact(dx, ref_dx, dtype)), defect


def test_entry_points_reject_host_tensors():
    """No GPU needed: the check comes before anything touches the device."""
    x = torch.zeros(4, 6)
    col = torch.zeros(3, dtype=torch.long)
    off = torch.tensor([0, 1, 3])
    for call in (lambda: _C.segment_mean_fwd(x, col, off, 2),
                 lambda: _C.segment_mean_cat_fwd(x, col, off, 2),
                 lambda: _C.segment_mean_bwd(x[:2], col, off, 4),
                 lambda: _C.segment_mean_cat_bwd(x[:2], col, off, 4),
                 lambda: _C.segment_wsum_fwd(x, col, off, None, None, None),
                 lambda: _C.segment_wsum_bwd(x[:2], None, col, off, None,
                                             None, None, 4, True, False,
                                             False, None)):
        with pytest.raises(RuntimeError, match="on device"):
            call()


# --------------------------------------------------------------------------
# GPU: the kernels
# --------------------------------------------------------------------------
def _run(case, cat, deterministic=False):
    from glt_amd.ops import (segment_mean, segment_mean_cat,
                             set_deterministic)

    fn = segment_mean_cat if cat else segment_mean
    x = case["x"].clone().requires_grad_(True)
    set_deterministic(deterministic)
    try:
        out = fn(x, case["tgt"], case["col"], case["n_tgt"])
        out.backward(_dy(case, cat))
    finally:
        set_deterministic(False)
    return out.detach(), x.grad


def _check_exact(case):
    dtype, n_tgt, F = case["dtype"], case["n_tgt"], case["F"]
    got = {}
    for cat in (False, True):
        ref_out, ref_dx, mag, _ = _reference(case, cat)
        assert mag.max().item() < 512      # inside the snap headroom
        out, dx = got[cat] = _run(case, cat)
        assert out.shape == ref_out.shape and dx.shape == case["x"].shape
        assert _exact(out, ref_out, dtype), "forward, cat=%s" % cat
        assert _exact(dx, ref_dx, dtype), "backward, cat=%s" % cat
        out_d, dx_d = _run(case, cat, deterministic=True)
        assert torch.equal(out_d, out)
        assert _exact(dx_d, ref_dx, dtype), "deterministic, cat=%s" % cat
    # cat: right half is the root rows, left half the plain mean; rows
    # past the targets get neighbour terms only, the others dy's right half
    (out, dx), (out_c, dx_c) = got[False], got[True]
    assert torch.equal(out_c[:, F:], case["x"][:n_tgt])
    assert torch.equal(out_c[:, :F], out)
    assert torch.equal(dx_c[n_tgt:], dx[n_tgt:])
    assert not torch.equal(dx_c[:n_tgt], dx[:n_tgt])
    if dtype == F32:    # a bf16 dx is rounded once, after the sum
        assert torch.equal(dx_c[:n_tgt], dx[:n_tgt] + case["dy"][:, F:])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F", SHAPES, ids=SHAPE_IDS)
def test_exact_bit_for_bit(dtype, F):
    _check_exact(_case(F, dtype, EXACT_DEGS, device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_cat_with_every_row_a_target(dtype):
    _check_exact(_case(100, dtype, EXACT_DEGS, n_src=N_TGT, seed=1,
                       device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_grid_stride(dtype):
    """8200 targets, at most 8192 resident waves: the last 8 targets are
    reached only by the stride loop."""
    _check_exact(_case(4, dtype, (0, 1, 2), n_tgt=8200, n_src=8300, seed=2,
                       device="cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F", SHAPES, ids=SHAPE_IDS)
def test_mixed_degrees_within_derived_bounds(dtype, F):
    case = _case(F, dtype, MIXED_DEGS, seed=3, device="cuda")
    for cat in (False, True):
        ref_out, ref_dx, mag, cnt = _reference(case, cat)
        out, dx = _run(case, cat)
        assert out.dtype == dtype and dx.dtype == dtype
        err = (out.double() - ref_out).abs()
        bound = (2.0 ** -22 if dtype == F32 else 2.0 ** -8) * ref_out.abs()
        print("fwd cat=%s: max err/bound %.3f" % (
            cat, (err / bound.clamp(min=1e-300)).max().item()))
        assert (err <= bound).all()
        if cat:
            assert torch.equal(out[:, F:], case["x"][:case["n_tgt"]])
        bound = (cnt.unsqueeze(1) + 2) * 2.0 ** -24 * mag
        if dtype == BF16:
            bound = 2.0 ** -8 * (ref_dx.abs() + bound) + bound
        err = (dx.double() - ref_dx).abs()
        print("dx  cat=%s: max err/bound %.3f" % (
            cat, (err / bound.clamp(min=1e-300)).max().item()))
        assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_no_targets(dtype):
    F = 6
    x = torch.ones(5, F, device="cuda", dtype=dtype)
    col = torch.zeros(0, dtype=torch.long, device="cuda")
    off = torch.zeros(1, dtype=torch.long, device="cuda")
    out = _C.segment_mean_fwd(x, col, off, 0)
    assert out.shape == (0, F) and out.dtype == dtype
    out = _C.segment_mean_cat_fwd(x, col, off, 0)
    assert out.shape == (0, 2 * F) and out.dtype == dtype
    for det in (False, True):
        dx = _C.segment_mean_bwd(x[:0], col, off, 5, det)
        assert dx.shape == (5, F) and dx.dtype == F32 and not dx.any()
        dx = _C.segment_mean_cat_bwd(x[:0].repeat(1, 2), col, off, 5, det)
        assert dx.shape == (5, F) and dx.dtype == F32 and not dx.any()


# --------------------------------------------------------------------------
# GPU: input validation.  Every call below must raise (or return) before
# any kernel is launched.
# --------------------------------------------------------------------------
def _valid_args():
    x = torch.zeros(6, 4, device="cuda")
    col = torch.zeros(5, dtype=torch.long, device="cuda")
    off = torch.tensor([0, 2, 5], device="cuda")
    return x, col, off


_ENTRY = {
    "mean_fwd": lambda x, col, off: _C.segment_mean_fwd(x, col, off, 2),
    "cat_fwd": lambda x, col, off: _C.segment_mean_cat_fwd(x, col, off, 2),
    "mean_bwd": lambda x, col, off: _C.segment_mean_bwd(x[:2], col, off, 6),
    "cat_bwd": lambda x, col, off: _C.segment_mean_cat_bwd(x[:2], col, off,
                                                          6),
}


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(_ENTRY))
def test_rejects_bad_index_tensors(entry):
    call = _ENTRY[entry]
    x, col, off = _valid_args()
    bad = [(x, col.int(), off), (x, col, off.int()),
           (x, col.cpu(), off), (x, col, off.cpu()),
           (x, col, off[:2]),                              # short offsets
           (x, col, torch.cat([off, off])),                # long offsets
           (x, col.repeat(2)[::2], off),                   # strided col
           (x, col, off.repeat_interleave(2)[::2])]        # strided offsets
    for args in bad:
        with pytest.raises(RuntimeError, match="segment"):
            call(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(_ENTRY))
def test_rejects_bad_values_tensor(entry):
    call = _ENTRY[entry]
    x, col, off = _valid_args()
    bad = [x.half(), x.double(), x.long(), x.cpu(), x.flatten(),
           x.unsqueeze(0)]
    if entry.endswith("fwd"):       # the backward makes dy contiguous
        bad.append(x.repeat(1, 2)[:, ::2])
    for v in bad:
        with pytest.raises(RuntimeError, match="segment"):
            call(v, col, off)


@pytest.mark.gpu
def test_rejects_bad_cat_shapes():
    x, col, off = _valid_args()
    with pytest.raises(RuntimeError, match="even"):       # odd dy width
        _C.segment_mean_cat_bwd(x[:2, :3], col, off, 6)
    with pytest.raises(RuntimeError, match="prefix"):     # n_src < n_tgt
        _C.segment_mean_cat_bwd(x[:2], col, off, 1)
    with pytest.raises(RuntimeError, match="prefix"):
        _C.segment_mean_cat_fwd(x[:1], col, off, 2)


@pytest.mark.gpu
def test_zero_channels():
    x, col, off = _valid_args()
    x = x[:, :0].contiguous()
    assert _C.segment_mean_fwd(x, col, off, 2).shape == (2, 0)
    assert _C.segment_mean_cat_fwd(x, col, off, 2).shape == (2, 0)
    for det in (False, True):
        assert _C.segment_mean_bwd(x[:2], col, off, 6, det).shape == (6, 0)
        assert _C.segment_mean_cat_bwd(x[:2], col, off, 6,
                                       det).shape == (6, 0)

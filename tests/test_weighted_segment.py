"""Weighted segment sum (ops.segment_weighted_sum) and edge-weighted
GCNConv / GCN.

    out[t, :] = a[t] * sum_{e in seg(t)} w[e] * b[col[e]] * x[col[e], :]
    dx[c, :] += a[t] * w[e] * b[c] * dy[t, :]          for every edge e=(t,c)
    dw[e]     = a[t] * b[c] * <dy[t, :], x[c, :]>

CPU tests (unmarked) cover the torch composition, the layer rule and the
model plumbing; GPU tests cover the HIP kernels against an fp64 reference.

Bounds used by the GPU tests.  They are forward-error bounds computed in
fp64 inside the tests, not tuned numbers.  u32 = 2^-23; any fp32
summation order of n terms errs by at most (n-1) * 2^-24 * sum|terms|,
and every factor product adds one rounding (2^-24 relative) per term:
  forward fp32: (deg_t + 5) * u32 * a_t * sum_e |w_e * b_c * x|
  forward bf16: 2^-8 * (|ref| + fp32 bound) + fp32 bound
                (one rounding of the fp32 accumulator to bf16; inputs are
                the bf16 values, which are exact in fp64)
  dx, plain   : (cnt_c + 5) * u32 * sum|terms|, cnt_c = in-batch
                in-degree of c.  A bf16 dx is the fp32 arena rounded once,
                so it gets the bf16 forward form over this bound.
  dw          : (F + 5) * u32 * |a_t * b_c| * sum_f |dy * x|
  dx, deterministic mode (H = 6 headroom bits, as kGridHeadroomBits):
                B = max|dy| * max|a| * max|w| * max|b|, 2^e > B,
                q = 2^(e + H - 24); per term snap <= q/2 plus three
                roundings of a value <= B; sums are exact while no dx
                element collects more than 2^H * 2^e, so
                err <= cnt * (q/2 + 3 * u32 * B) and the bits do not depend
                on the order.
Layer tests use the existing torch composition and fp64 as the yardstick:
the fused path's max error against the fp64 module must be at most twice
the composite path's own error (+ 1e-6 * max|ref| when that is ~0).
"""
import copy
import math

import pytest
import torch

import glt_amd
from glt_amd import Dataset, NeighborLoader
from glt_amd.models import GCN
from glt_amd.models.layers import GCNConv

U32 = 2.0 ** -23
UBF = 2.0 ** -8
H = 6
COMBOS = ["none", "w", "ab", "wab"]


# --------------------------------------------------------------------------
# shared helpers
# --------------------------------------------------------------------------
def _factors(combo, w, a, b):
    return (w if "w" in combo else None, a if "a" in combo else None,
            b if "b" in combo else None)


def _coef(tgt, src, w, a, b, with_w=True):
    """fp64 per-edge coefficient a[t] * w[e] * b[c] (absent factor = 1)."""
    c = torch.ones(tgt.numel(), dtype=torch.float64, device=tgt.device)
    if a is not None:
        c = c * a.double()[tgt]
    if b is not None:
        c = c * b.double()[src]
    if w is not None and with_w:
        c = c * w.double()
    return c


def _ref_fwd(x, tgt, src, n_tgt, w, a, b):
    """fp64 (out, sum of |terms|) by scatter."""
    c = _coef(tgt, src, w, a, b).unsqueeze(1)
    terms = c * x.double()[src]
    out = torch.zeros(n_tgt, x.size(1), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    out.index_add_(0, tgt, terms)
    mag.index_add_(0, tgt, terms.abs())
    return out, mag


def _ref_bwd(x, dy, tgt, src, w, a, b):
    """fp64 (dx, sum|dx terms|, dw, |a b| sum_f |dy x|)."""
    c = _coef(tgt, src, w, a, b).unsqueeze(1)
    terms = c * dy.double()[tgt]
    dx = torch.zeros(x.size(0), x.size(1), dtype=torch.float64,
                     device=x.device)
    dmag = torch.zeros_like(dx)
    dx.index_add_(0, src, terms)
    dmag.index_add_(0, src, terms.abs())
    ab = _coef(tgt, src, w, a, b, with_w=False)
    prod = dy.double()[tgt] * x.double()[src]
    return dx, dmag, ab * prod.sum(1), ab.abs() * prod.abs().sum(1)


def _wide(shape, gen, device):
    """Magnitudes spread over four decades."""
    mag = 10.0 ** (-4.0 * torch.rand(shape, generator=gen, device=device))
    return torch.randn(shape, generator=gen, device=device) * mag


# --------------------------------------------------------------------------
# CPU: composite op
# --------------------------------------------------------------------------
def _cpu_case(seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    n_src, n_tgt, E, F = 13, 9, 40, 5
    tgt = torch.randint(0, n_tgt - 2, (E,), generator=g)  # unsorted, and
    src = torch.randint(0, n_src, (E,), generator=g)      # n_tgt past last
    x = torch.randn(n_src, F, generator=g, dtype=dtype)
    w = torch.rand(E, generator=g, dtype=dtype) * 2
    a = torch.rand(n_tgt, generator=g, dtype=dtype) + 0.1
    b = torch.rand(n_src, generator=g, dtype=dtype) + 0.1
    return x, tgt, src, n_tgt, w, a, b


@pytest.mark.parametrize("combo", COMBOS)
def test_composite_matches_dense_reference(combo):
    from glt_amd.ops import segment_weighted_sum

    x, tgt, src, n_tgt, w, a, b = _cpu_case()
    w_, a_, b_ = _factors(combo, w, a, b)
    out = segment_weighted_sum(x, tgt, src, n_tgt, w_, a_, b_,
                               sorted_by_target=False)
    # dense: A[t, c] = sum of the coefficients of the edges (t, c)
    A = torch.zeros(n_tgt, x.size(0), dtype=torch.float64)
    A.index_put_((tgt, src), _coef(tgt, src, w_, None, b_), accumulate=True)
    ref = A @ x
    if a_ is not None:
        ref = a_.unsqueeze(1) * ref
    assert out.shape == (n_tgt, x.size(1)) and out.dtype == x.dtype
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    assert not out[n_tgt - 2:].any()
    # fp32 input with fp64 / bf16 factors keeps x's dtype
    o32 = segment_weighted_sum(
        x.float(), tgt, src, n_tgt, w_,
        None if a_ is None else a_.to(torch.bfloat16).double(),
        None if b_ is None else b_.float(), sorted_by_target=False)
    assert o32.dtype == torch.float32


@pytest.mark.parametrize("combo", COMBOS)
def test_composite_gradcheck(combo):
    from glt_amd.ops import segment_weighted_sum

    x, tgt, src, n_tgt, w, a, b = _cpu_case(1)
    w_, a_, b_ = _factors(combo, w, a, b)
    x.requires_grad_(True)
    if w_ is not None:
        w_.requires_grad_(True)
        assert torch.autograd.gradcheck(
            lambda xx, ww: segment_weighted_sum(
                xx, tgt, src, n_tgt, ww, a_, b_, sorted_by_target=False),
            (x, w_))
    else:
        assert torch.autograd.gradcheck(
            lambda xx: segment_weighted_sum(
                xx, tgt, src, n_tgt, None, a_, b_, sorted_by_target=False),
            (x,))


def test_scale_requiring_grad_raises():
    from glt_amd.ops import segment_weighted_sum

    x, tgt, src, n_tgt, w, a, b = _cpu_case(2)
    with pytest.raises(ValueError):
        segment_weighted_sum(x, tgt, src, n_tgt, w,
                             a.clone().requires_grad_(True), b,
                             sorted_by_target=False)
    with pytest.raises(ValueError):
        segment_weighted_sum(x, tgt, src, n_tgt, w, a,
                             b.clone().requires_grad_(True))


# --------------------------------------------------------------------------
# CPU: GCNConv with weights
# --------------------------------------------------------------------------
def _parent_gcnconv(conv, x, edge_index, nt):
    """Literal copy of the unweighted GCNConv.forward before edge weights."""
    n = x.size(0)
    tgt, src = edge_index[0], edge_index[1]
    deg = torch.bincount(torch.cat([tgt, src]),
                         minlength=n).clamp_(min=1).to(x.dtype)
    norm = deg.rsqrt()
    h = conv.lin(x)
    msg = h.index_select(0, src) * norm[src].unsqueeze(1)
    out = h.new_zeros(nt, h.size(1))
    out.index_add_(0, tgt, msg)
    return out * norm[:nt].unsqueeze(1)


def _layer_case(seed=3):
    g = torch.Generator().manual_seed(seed)
    n, nt, E = 30, 12, 90
    tgt = torch.randint(0, nt, (E,), generator=g)
    src = torch.randint(0, n - 1, (E,), generator=g)  # node n-1 is isolated
    x = torch.randn(n, 8, generator=g)
    torch.manual_seed(seed)
    return GCNConv(8, 6), x, torch.stack([tgt, src]), nt


def test_gcnconv_unweighted_bit_identical_to_parent_formula():
    conv, x, ei, nt = _layer_case()
    assert torch.equal(conv(x, ei, nt), _parent_gcnconv(conv, x, ei, nt))
    assert torch.equal(conv(x, ei), _parent_gcnconv(conv, x, ei, x.size(0)))
    # sorted_by_target on the CPU is still the composition
    assert torch.equal(conv(x, ei, nt, sorted_by_target=True),
                       _parent_gcnconv(conv, x, ei, nt))


def test_gcnconv_unit_weights_bit_identical_to_unweighted():
    conv, x, ei, nt = _layer_case(4)
    ones = torch.ones(ei.size(1))
    assert torch.equal(conv(x, ei, nt, edge_weight=ones), conv(x, ei, nt))
    assert torch.equal(conv(x, ei, edge_weight=ones), conv(x, ei))


def test_gcnconv_weighted_matches_dense_reference():
    conv, x, ei, nt = _layer_case(5)
    g = torch.Generator().manual_seed(6)
    E, n = ei.size(1), x.size(0)
    w = torch.rand(E, generator=g)
    w[::7] = 0.0
    # all edges of node 3 (either end) get weight 0: degree 0 -> norm 0
    w[(ei[0] == 3) | (ei[1] == 3)] = 0.0
    out = conv(x, ei, nt, edge_weight=w)

    c64 = copy.deepcopy(conv).double()
    wd, tgt, src = w.double(), ei[0], ei[1]
    deg = torch.zeros(n, dtype=torch.float64)
    for e in range(E):
        deg[tgt[e]] += wd[e]
        deg[src[e]] += wd[e]
    assert deg[3] == 0 and deg[n - 1] == 0
    norm = torch.where(deg > 0, deg.clamp(min=1e-300) ** -0.5,
                       torch.zeros_like(deg))
    A = torch.zeros(nt, n, dtype=torch.float64)
    for e in range(E):
        A[tgt[e], src[e]] += norm[tgt[e]] * wd[e] * norm[src[e]]
    ref = A @ c64.lin(x.double())
    assert torch.isfinite(out).all()
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=1e-6)
    assert not out[3].any()
    # gradients reach x and the edge weight
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    conv(xg, ei, nt, edge_weight=wg).sum().backward()
    assert xg.grad is not None and wg.grad is not None
    assert wg.grad.shape == w.shape and wg.grad.dtype == w.dtype


# --------------------------------------------------------------------------
# CPU: GCN with trim lists over a loader batch
# --------------------------------------------------------------------------
def test_gcn_trim_lists_with_edge_weight(ring_graph):
    glt_amd.seed_everything(7)
    n = ring_graph["num_nodes"]
    ew = torch.rand(2 * n) + 0.05
    ds = Dataset()
    ds.init_graph(edge_index=ring_graph["edge_index"], graph_mode="CPU",
                  num_nodes=n)
    ds.init_node_features(ring_graph["feats"], with_gpu=False)
    ds.init_edge_features(ew[:, None], with_gpu=False)
    ds.init_node_labels(ring_graph["labels"])
    loader = NeighborLoader(ds, [2, 2], input_nodes=torch.arange(n),
                            batch_size=5, shuffle=True, with_edge=True)
    data = next(iter(loader))
    w = data.edge_attr[:, 0]
    assert torch.equal(w, ew[data.edge])
    # loader batches are target-ascending across hops
    assert (data.edge_index[0][1:] >= data.edge_index[0][:-1]).all()

    torch.manual_seed(8)
    model = GCN(16, 8, 2, out_channels=4)
    x = data.x / n
    out = model(x, data.edge_index, data.num_sampled_nodes,
                data.num_sampled_edges, edge_weight=w)
    nsn = [int(v) for v in data.num_sampled_nodes]
    nse = [int(v) for v in data.num_sampled_edges]
    h = model.convs[0](x[:sum(nsn[:3])], data.edge_index[:, :sum(nse[:2])],
                       num_target=sum(nsn[:2]),
                       edge_weight=w[:sum(nse[:2])])
    h = torch.relu(h)
    h = model.convs[1](h[:sum(nsn[:2])], data.edge_index[:, :nse[0]],
                       num_target=nsn[0], edge_weight=w[:nse[0]])
    assert out.shape == (nsn[0], 4)
    assert torch.equal(out, h)
    # and the weights matter
    assert not torch.equal(out, model(x, data.edge_index,
                                      data.num_sampled_nodes,
                                      data.num_sampled_edges))


# --------------------------------------------------------------------------
# GPU: kernels against the fp64 reference
# --------------------------------------------------------------------------
_case_cache = {}


def _kernel_case(F, dtype):
    """Degree patterns that reach every branch: empty / single-edge
    segments, the 8-deep batch boundary, the wave width, one long hub,
    ordinary rows and trailing empty targets.  Built once per (F, dtype)
    and never modified."""
    key = (F, dtype)
    if key in _case_cache:
        return _case_cache[key]
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(100 + F)
    gc = torch.Generator().manual_seed(200 + F)
    deg = torch.cat([torch.tensor([0, 1, 8, 9, 17, 64, 65, 1000]),
                     torch.randint(0, 12, (290,), generator=gc),
                     torch.zeros(3, dtype=torch.long)]).to(dev)
    n_tgt, n_src = deg.numel(), 700
    tgt = torch.repeat_interleave(torch.arange(n_tgt, device=dev), deg)
    E = tgt.numel()
    src = torch.randint(0, n_src, (E,), generator=g, device=dev)
    x = _wide((n_src, F), g, dev).to(dtype)
    dy = _wide((n_tgt, F), g, dev).to(dtype)
    w = torch.rand(E, generator=g, device=dev) * 2
    w[torch.rand(E, generator=g, device=dev) < 0.1] = 0.0
    a = torch.rand(n_tgt, generator=g, device=dev) + 0.1
    b = torch.rand(n_src, generator=g, device=dev) + 0.1
    case = dict(x=x, dy=dy, tgt=tgt, src=src, n_tgt=n_tgt, w=w, a=a, b=b,
                deg=deg.double(),
                cnt=torch.bincount(src, minlength=n_src).double())
    _case_cache[key] = case
    return case


def _low_precision(bound, ref, dtype):
    """Bound of a result held in `dtype` given the fp32 bound."""
    if dtype == torch.bfloat16:
        return UBF * (ref.abs() + bound) + bound
    return bound


def _check_kernels(case, combo, dtype):
    from glt_amd.ops import segment_weighted_sum

    x, dy, tgt, src, n_tgt = (case[k] for k in
                              ("x", "dy", "tgt", "src", "n_tgt"))
    w, a, b = _factors(combo, case["w"], case["a"], case["b"])
    F = x.size(1)
    runs = []
    for _ in range(3):
        xx = x.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True) if w is not None else None
        out = segment_weighted_sum(xx, tgt, src, n_tgt, ww, a, b)
        out.backward(dy)
        runs.append((out.detach(), xx.grad, None if ww is None else ww.grad))
    out, dx, dw = runs[0]
    assert out.dtype == dtype and out.shape == (n_tgt, F)
    assert dx.dtype == dtype and dx.shape == x.shape
    # the forward has no atomics: same bits every run
    assert torch.equal(out, runs[1][0]) and torch.equal(out, runs[2][0])

    ref, mag = _ref_fwd(x, tgt, src, n_tgt, w, a, b)
    fb = (case["deg"].unsqueeze(1) + 5) * U32 * mag
    bound = _low_precision(fb, ref, dtype)
    err = (out.double() - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print("fwd %s F=%d %s: max err/bound %.3f" % (combo, F, dtype, ratio))
    assert (err <= bound).all()
    assert not out[case["deg"] == 0].any()

    rdx, dmag, rdw, wmag = _ref_bwd(x, dy, tgt, src, w, a, b)
    db = _low_precision((case["cnt"].unsqueeze(1) + 5) * U32 * dmag, rdx,
                        dtype)
    err = (dx.double() - rdx).abs()
    ratio = (err / db.clamp(min=1e-300)).max().item()
    print("dx  %s F=%d %s: max err/bound %.3f" % (combo, F, dtype, ratio))
    assert (err <= db).all()

    if w is not None:
        assert dw.dtype == w.dtype and dw.shape == w.shape
        assert torch.equal(dw, runs[1][2]) and torch.equal(dw, runs[2][2])
        wb = (F + 5) * U32 * wmag
        err = (dw.double() - rdw).abs()
        ratio = (err / wb.clamp(min=1e-300)).max().item()
        print("dw  %s F=%d %s: max err/bound %.3f" % (combo, F, dtype,
                                                      ratio))
        assert (err <= wb).all()


@pytest.mark.gpu
@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F", [1, 7, 128, 130])
def test_kernels_match_fp64_reference(F, dtype, combo):
    _check_kernels(_kernel_case(F, dtype), combo, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernels_grid_stride(dtype):
    """More targets than resident waves (8192): the grid-stride loop."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(9)
    n_tgt, n_src, F = 9000, 700, 4
    deg = torch.randint(0, 4, (n_tgt,), generator=g, device=dev)
    tgt = torch.repeat_interleave(torch.arange(n_tgt, device=dev), deg)
    E = tgt.numel()
    case = dict(
        x=_wide((n_src, F), g, dev).to(dtype),
        dy=_wide((n_tgt, F), g, dev).to(dtype), tgt=tgt,
        src=torch.randint(0, n_src, (E,), generator=g, device=dev),
        n_tgt=n_tgt, w=torch.rand(E, generator=g, device=dev) * 2,
        a=torch.rand(n_tgt, generator=g, device=dev) + 0.1,
        b=torch.rand(n_src, generator=g, device=dev) + 0.1,
        deg=deg.double())
    case["cnt"] = torch.bincount(case["src"], minlength=n_src).double()
    _check_kernels(case, "wab", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deterministic_mode_bit_reproducible_and_bounded(dtype):
    from glt_amd.ops import (is_deterministic, segment_weighted_sum,
                             set_deterministic)

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(10)
    n_tgt, n_src, deg, F = 4000, 4100, 10, 130
    tgt = torch.arange(n_tgt, device=dev).repeat_interleave(deg)
    E = tgt.numel()
    src = torch.randint(0, n_src, (E,), generator=g, device=dev)
    cnt = torch.bincount(src, minlength=n_src).double()
    assert cnt.max().item() <= 2 ** H  # inside the headroom condition
    x = _wide((n_src, F), g, dev).to(dtype)
    mag = 10.0 ** (-6.0 * torch.rand(n_tgt, F, generator=g, device=dev))
    dy = (torch.randn(n_tgt, F, generator=g, device=dev) * mag).to(dtype)
    w = torch.rand(E, generator=g, device=dev) * 1.99 + 0.005
    a = torch.rand(n_tgt, generator=g, device=dev) * 1.99 + 0.005
    b = torch.rand(n_src, generator=g, device=dev) * 1.99 + 0.005

    def grad():
        xx = x.clone().requires_grad_(True)
        segment_weighted_sum(xx, tgt, src, n_tgt, w, a, b).backward(dy)
        return xx.grad

    rdx, dmag, _, _ = _ref_bwd(x, dy, tgt, src, w, a, b)
    assert not is_deterministic()
    plain = grad()
    pb = _low_precision((cnt.unsqueeze(1) + 5) * U32 * dmag, rdx, dtype)
    assert ((plain.double() - rdx).abs() <= pb).all()

    set_deterministic(True)
    try:
        runs = [grad() for _ in range(3)]
    finally:
        set_deterministic(False)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    B = (dy.double().abs().max() * a.double().max() * w.double().max()
         * b.double().max()).item()
    e = math.frexp(B)[1]            # 2^(e-1) <= B < 2^e
    q = 2.0 ** (e + H - 24)
    bound = _low_precision(
        (cnt * (q / 2 + 3 * U32 * B)).unsqueeze(1).expand_as(rdx), rdx,
        dtype)
    err = (runs[0].double() - rdx).abs()
    print("det %s: max err %.3e, max bound %.3e, B %.3e" % (
        dtype, err.max().item(), bound.max().item(), B))
    assert (err <= bound).all()


@pytest.mark.gpu
def test_edge_cases(monkeypatch):
    from glt_amd.ops import segment, segment_weighted_sum

    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(11)
    F = 33
    x = torch.randn(50, F, generator=g, device=dev)
    b = torch.rand(50, generator=g, device=dev) + 0.1
    none = torch.zeros(0, dtype=torch.long, device=dev)

    # E = 0
    xx = x.clone().requires_grad_(True)
    ww = torch.zeros(0, device=dev, requires_grad=True)
    out = segment_weighted_sum(xx, none, none, 4, ww,
                               torch.ones(4, device=dev), b)
    assert out.shape == (4, F) and not out.any()
    out.sum().backward()
    assert not xx.grad.any() and ww.grad.shape == (0,)

    # n_tgt = 0
    xx = x.clone().requires_grad_(True)
    out = segment_weighted_sum(xx, none, none, 0, None, None, b)
    assert out.shape == (0, F)
    out.sum().backward()
    assert xx.grad.shape == x.shape and not xx.grad.any()

    # x needs no gradient, the edge weight does
    deg = torch.randint(0, 6, (40,), generator=g, device=dev)
    tgt = torch.repeat_interleave(torch.arange(40, device=dev), deg)
    E = tgt.numel()
    src = torch.randint(0, 50, (E,), generator=g, device=dev)
    w = torch.rand(E, generator=g, device=dev)
    a = torch.rand(40, generator=g, device=dev) + 0.1
    dy = torch.randn(40, F, generator=g, device=dev)
    ww = w.clone().requires_grad_(True)
    segment_weighted_sum(x, tgt, src, 40, ww, a, b).backward(dy)
    _, _, rdw, wmag = _ref_bwd(x, dy, tgt, src, w, a, b)
    assert ((ww.grad.double() - rdw).abs() <= (F + 5) * U32 * wmag).all()
    # a half-precision weight gets its gradient back in its own dtype
    wh = w.to(torch.bfloat16).requires_grad_(True)
    segment_weighted_sum(x, tgt, src, 40, wh, a, b).backward(dy)
    assert wh.grad.dtype == torch.bfloat16 and wh.grad.shape == w.shape

    # shuffled edges with sorted_by_target=False: the composition, and
    # still the reference (any fp32 summation order is inside the bound)
    def no_kernel(*args, **kw):
        raise AssertionError("fused path taken for unsorted edges")

    perm = torch.randperm(E, generator=g, device=dev)
    with monkeypatch.context() as m:
        m.setattr(segment._SegmentWeightedSum, "apply", no_kernel)
        out = segment_weighted_sum(x, tgt[perm], src[perm], 40, w[perm], a,
                                   b, sorted_by_target=False)
    ref, mag = _ref_fwd(x, tgt, src, 40, w, a, b)
    assert ((out.double() - ref).abs()
            <= (deg.double().unsqueeze(1) + 5) * U32 * mag).all()


# --------------------------------------------------------------------------
# GPU: layer and model
# --------------------------------------------------------------------------
def _gpu_layer_case(seed, n=600, nt=200, mean_deg=8):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(mean_deg - 4, mean_deg + 5, (nt,), generator=g)
    tgt = torch.repeat_interleave(torch.arange(nt), deg)
    E = tgt.numel()
    src = torch.randint(0, n, (E,), generator=g)
    x = torch.randn(n, 64, generator=g)
    w = torch.rand(E, generator=g) + 0.05
    gy = torch.randn(nt, 32, generator=g)
    torch.manual_seed(seed)
    return GCNConv(64, 32), x, torch.stack([tgt, src]), nt, w, gy


def _run_layer(conv, x, ei, nt, w, gy, **kw):
    conv.zero_grad()
    xx = x.clone().requires_grad_(True)
    ww = w.clone().requires_grad_(True) if w is not None else None
    out = conv(xx, ei, nt, edge_weight=ww, **kw)
    out.backward(gy.to(out.dtype))
    res = {"out": out.detach(), "dx": xx.grad,
           "dW": conv.lin.weight.grad.clone()}
    if ww is not None:
        res["dw"] = ww.grad
    return res


def _within_twice(name, fused, comp, ref):
    ef = (fused.double().cpu() - ref).abs().max().item()
    ec = (comp.double().cpu() - ref).abs().max().item()
    print("%s: fused err %.3e, composite err %.3e" % (name, ef, ec))
    assert ef <= 2 * ec + 1e-6 * ref.abs().max().item(), name


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
def test_gcnconv_fused_vs_composite_vs_fp64(weighted):
    conv, x, ei, nt, w, gy = _gpu_layer_case(12)
    if not weighted:
        w = None
    c64 = copy.deepcopy(conv).double()
    ref = _run_layer(c64, x.double(), ei, nt,
                     None if w is None else w.double(), gy.double())
    conv = conv.cuda()
    args = (x.cuda(), ei.cuda(), nt, None if w is None else w.cuda(),
            gy.cuda())
    fused = _run_layer(conv, *args, sorted_by_target=True)
    comp = _run_layer(conv, *args, sorted_by_target=False)
    for k in ref:
        _within_twice(k, fused[k], comp[k], ref[k])


@pytest.mark.gpu
def test_gcnconv_bf16_fused_no_worse_than_composite():
    """bf16 storage with fp32 accumulation must beat bf16 atomics."""
    conv, x, ei, nt, w, gy = _gpu_layer_case(13, mean_deg=12)
    x16 = x.to(torch.bfloat16)
    c64 = copy.deepcopy(conv).double()
    conv = conv.cuda()
    for ww in (None, w):
        with torch.no_grad():
            ref = c64(x16.double(), ei, nt,
                      edge_weight=None if ww is None else ww.double())
            wc = None if ww is None else ww.cuda()
            fused = conv(x16.cuda(), ei.cuda(), nt, edge_weight=wc,
                         sorted_by_target=True)
            comp = conv(x16.cuda(), ei.cuda(), nt, edge_weight=wc,
                        sorted_by_target=False)
        assert fused.dtype == torch.bfloat16
        ef = (fused.double().cpu() - ref).abs().max().item()
        ec = (comp.double().cpu() - ref).abs().max().item()
        print("bf16 weighted=%s: fused err %.3e, composite err %.3e" % (
            ww is not None, ef, ec))
        assert ef <= ec


def _gpu_weighted_dataset(n, E, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (E,), generator=g)
    dst = torch.randint(0, n, (E,), generator=g)
    ew = 1.0 - torch.rand(E, generator=g)          # (0, 1]
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack([src, dst]), graph_mode="CUDA",
                  num_nodes=n, device=0)
    ds.init_node_features(torch.randn(n, 32, generator=g), split_ratio=1.0,
                          device=0)
    ds.init_edge_features(ew[:, None], split_ratio=1.0, device=0)
    ds.init_node_labels(torch.randint(0, 5, (n,), generator=g))
    return ds, ew


@pytest.mark.gpu
def test_gcn_engages_fused_path_on_loader_batches(monkeypatch):
    import glt_amd.ops as ops

    dev = torch.device("cuda", 0)
    glt_amd.seed_everything(14)
    ds, _ = _gpu_weighted_dataset(2000, 16000, 14)
    loader = NeighborLoader(ds, [4, 4], input_nodes=torch.arange(128),
                            batch_size=64, device=dev, to_device=dev,
                            with_edge=True)
    data = next(iter(loader))
    model = GCN(32, 16, 2, out_channels=5).to(dev)
    calls = []
    real = ops.segment_weighted_sum

    def counting(x, tgt, src, n_tgt, edge_weight=None, tgt_scale=None,
                 src_scale=None, sorted_by_target=True):
        calls.append(bool(sorted_by_target))
        return real(x, tgt, src, n_tgt, edge_weight, tgt_scale, src_scale,
                    sorted_by_target)

    monkeypatch.setattr(ops, "segment_weighted_sum", counting)
    model(data.x, data.edge_index, data.num_sampled_nodes,
          data.num_sampled_edges, edge_weight=data.edge_attr[:, 0])
    assert calls == [True, True]
    del calls[:]
    model(data.x, data.edge_index, edge_weight=data.edge_attr[:, 0])
    assert calls == [False, False]


@pytest.mark.gpu
def test_gcn_weighted_end_to_end():
    dev = torch.device("cuda", 0)
    glt_amd.seed_everything(15)
    ds, ew = _gpu_weighted_dataset(2000, 16000, 15)
    loader = NeighborLoader(ds, [5, 5], input_nodes=torch.arange(256),
                            batch_size=128, device=dev, to_device=dev,
                            with_edge=True)
    data = next(iter(loader))
    w = data.edge_attr[:, 0]
    assert torch.equal(w.cpu(), ew[data.edge.cpu()])
    model = GCN(32, 16, 2, out_channels=5).to(dev)
    trims = (data.num_sampled_nodes, data.num_sampled_edges)
    bs = data.batch_size

    logits = {}
    for dtype in (torch.float32, torch.bfloat16):
        model.zero_grad()
        out = model(data.x.to(dtype), data.edge_index, *trims,
                    edge_weight=w)[:bs]
        loss = torch.nn.functional.cross_entropy(out.float(), data.y[:bs])
        loss.backward()
        assert torch.isfinite(loss)
        for p in model.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all()
        logits[dtype] = out.detach()

    # same batch on the CPU: fp64 is the reference, the fp32 composition
    # the yardstick
    cpu = copy.deepcopy(model).cpu()
    xc, eic, wc = data.x.cpu(), data.edge_index.cpu(), w.cpu()
    with torch.no_grad():
        comp = cpu(xc, eic, *trims, edge_weight=wc)[:bs]
        ref = cpu.double()(xc.double(), eic, *trims,
                           edge_weight=wc.double())[:bs]
    _within_twice("logits", logits[torch.float32], comp, ref)

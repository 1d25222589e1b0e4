"""Segment max / min with the arg of the winner (ops.segment_max,
segment_min, segment_max_cat, segment_min_cat, segment_sum) and
SAGEConv / GraphSAGE ``aggr=``.

    out[t, f] = max (min) over e in seg(t) of x[col[e], f]
    arg[t, f] = col[e*], e* the FIRST edge of seg(t), in edge order, that
                attains it (strict compare, started from the first edge;
                a NaN wins and stays; empty segment: out 0, arg -1)
    dx[arg[t, f], f] += dy[t, f]        (+ dx[t, :] += dy[t, F:] for cat)

CPU tests (unmarked) pin the torch composition against a brute-force loop
and cover the layer and model plumbing.  GPU tests compare the HIP kernels
with that composition run in fp64 on the CPU, cast to the output dtype.

The forward is a selection, so it is compared bit for bit.  Bounds of the
backward tests, computed in fp64 inside the tests (u = 2^-24):
  integer dy in [-4, 4]: every partial sum is a small integer, exact in
                fp32 in any order, so dx is compared bit for bit, in plain
                and in deterministic mode (grid 2^-15, headroom 512).
  plain, fp32 : (cnt - 1) * u * sum|terms|, cnt = number of (t, f) whose
                arg is that row (+ 1 on root rows for cat): any summation
                order of cnt terms starting from an exact 0.
  bf16        : 2^-8 * (|ref| + b32) + b32 (the fp32 arena rounded once).
  deterministic: B = max|dy|, 2^e > B, q = 2^(e + 6 - 24); each term is
                snapped by at most q/2 after one rounding of a value <= B,
                sums are exact while cnt <= 64: cnt * (q/2 + u * B), and
                two runs give the same bits.
Layer and model tests use the yardstick rule of test_weighted_segment.py:
the fused path's max error against fp64 is at most twice the torch
composition's own error, plus 1e-6 * max|ref|.
"""
import copy
import math

import pytest
import torch

import glt_amd
from glt_amd import Dataset, NeighborLoader
from glt_amd.models import GraphSAGE
from glt_amd.models.layers import SAGEConv

U24 = 2.0 ** -24
UBF = 2.0 ** -8
H = 6
VARIANTS = [(True, False), (False, False), (True, True), (False, True)]


def _op(is_max, cat):
    from glt_amd import ops

    return {(True, False): ops.segment_max, (False, False): ops.segment_min,
            (True, True): ops.segment_max_cat,
            (False, True): ops.segment_min_cat}[(is_max, cat)]


# --------------------------------------------------------------------------
# brute force
# --------------------------------------------------------------------------
def _loop(x, tgt, src, n_tgt, is_max):
    """(out, arg) by the definition, one edge at a time."""
    F = x.size(1)
    out = torch.zeros(n_tgt, F, dtype=x.dtype)
    arg = torch.full((n_tgt, F), -1, dtype=torch.long)
    for t in range(n_tgt):
        for f in range(F):
            best = None
            for e in range(tgt.numel()):
                if int(tgt[e]) != t:
                    continue
                v = x[src[e], f].item()
                if best is None or (v > best if is_max else v < best) or \
                        (v != v and best == best):
                    best = v
                    arg[t, f] = src[e]
            if best is not None:
                out[t, f] = best
    return out, arg


def _loop_grad(arg, dy, n_src, cat):
    n_tgt, F = arg.shape
    dx = torch.zeros(n_src, F, dtype=dy.dtype)
    for t in range(n_tgt):
        for f in range(F):
            if arg[t, f] >= 0:
                dx[arg[t, f], f] += dy[t, f]
            if cat:
                dx[t, f] += dy[t, F + f]
    return dx


def _cpu_case(seed=0, ties=True):
    g = torch.Generator().manual_seed(seed)
    n_src, n_tgt, E, F = 13, 9, 40, 5
    tgt = torch.randint(0, n_tgt - 2, (E,), generator=g)  # unsorted, the
    src = torch.randint(0, n_src, (E,), generator=g)      # last two empty
    if ties:
        x = torch.randint(-1, 2, (n_src, F), generator=g).double()
    else:
        x = torch.randn(n_src, F, generator=g, dtype=torch.float64)
    return x, tgt, src, n_tgt


# --------------------------------------------------------------------------
# CPU: the torch composition
# --------------------------------------------------------------------------
@pytest.mark.parametrize("is_max,cat", VARIANTS)
def test_fallback_matches_brute_force(is_max, cat):
    from glt_amd.ops.segment import _segment_ext_arg

    x, tgt, src, n_tgt = _cpu_case()
    F = x.size(1)
    assert (torch.bincount(tgt, minlength=n_tgt)[-2:] == 0).all()
    ref, rarg = _loop(x, tgt, src, n_tgt, is_max)
    xx = x.clone().requires_grad_(True)
    out = _op(is_max, cat)(xx, tgt, src, n_tgt, sorted_by_target=False)
    arg = _segment_ext_arg(x, tgt, src, n_tgt, is_max)
    assert out.shape == (n_tgt, 2 * F if cat else F) and out.dtype == x.dtype
    assert torch.equal(arg, rarg)
    assert (arg[-2:] == -1).all() and not out[-2:, :F].any()
    assert torch.equal(out[:, :F], ref)
    if cat:
        assert torch.equal(out[:, F:], x[:n_tgt])
    g = torch.Generator().manual_seed(1)
    dy = torch.randint(-4, 5, out.shape, generator=g).double()
    out.backward(dy)
    assert torch.equal(xx.grad, _loop_grad(rarg, dy, x.size(0), cat))
    # sorted_by_target=True on the CPU is still the composition
    assert torch.equal(_op(is_max, cat)(x, tgt, src, n_tgt), out.detach())


@pytest.mark.parametrize("is_max,cat", VARIANTS)
def test_fallback_gradcheck(is_max, cat):
    x, tgt, src, n_tgt = _cpu_case(2, ties=False)
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda xx: _op(is_max, cat)(xx, tgt, src, n_tgt,
                                    sorted_by_target=False), (x,))


def test_fallback_nan_and_infinities():
    from glt_amd.ops import segment_max, segment_min
    from glt_amd.ops.segment import _segment_ext_arg

    inf, nan = float("inf"), float("nan")
    #          row 0       1          2          3          4
    x = torch.tensor([[1.0, -inf], [nan, -inf], [5.0, -inf], [nan, 2.0],
                      [7.0, -inf]], dtype=torch.float64)
    tgt = torch.tensor([0, 0, 0, 0, 1, 1, 2])
    src = torch.tensor([0, 2, 1, 3, 4, 0, 1])
    for op, is_max in ((segment_max, True), (segment_min, False)):
        xx = x.clone().requires_grad_(True)
        out = op(xx, tgt, src, 4, sorted_by_target=False)
        arg = _segment_ext_arg(x, tgt, src, 4, is_max)
        ref, rarg = _loop(x, tgt, src, 4, is_max)
        assert torch.equal(arg, rarg)
        assert torch.equal(out.isnan(), ref.isnan())
        assert torch.equal(out.nan_to_num(nan=123.0),
                           ref.nan_to_num(nan=123.0))
        # column 0 of target 0 holds NaNs in rows 1 and 3: first NaN edge
        assert out[0, 0].isnan() and arg[0, 0] == 1
        assert out[2, 0].isnan() and arg[2, 0] == 1
        out.backward(torch.ones_like(out))
        assert torch.equal(xx.grad, _loop_grad(rarg, torch.ones_like(out),
                                               5, False))
        assert xx.grad[1, 0] == 2 and xx.grad[3, 0] == 0
        assert not out[3].any() and (arg[3] == -1).all()
    out = segment_max(x, tgt, src, 4, sorted_by_target=False)
    arg = _segment_ext_arg(x, tgt, src, 4, True)
    # target 1, column 1: every value is -inf -> -inf (not 0), first edge
    assert out[1, 1] == -inf and arg[1, 1] == 4
    assert out[0, 1] == 2.0 and arg[0, 1] == 3


def test_fallback_without_edges_or_sources():
    """A relation that sampled nothing: no edges, possibly no source rows."""
    from glt_amd.ops import segment_max, segment_min_cat

    none = torch.zeros(0, dtype=torch.long)
    for n_src in (0, 4):
        x = torch.randn(n_src, 3, requires_grad=True)
        out = segment_max(x, none, none, 2, sorted_by_target=False)
        assert out.shape == (2, 3) and not out.any()
    x = torch.randn(4, 3, requires_grad=True)
    out = segment_min_cat(x, none, none, 2, sorted_by_target=False)
    assert not out[:, :3].any() and torch.equal(out[:, 3:], x[:2])
    out.sum().backward()
    assert torch.equal(x.grad[:2], torch.ones(2, 3)) and not x.grad[2:].any()


def test_segment_sum_is_unweighted_weighted_sum():
    from glt_amd.ops import segment_sum, segment_weighted_sum

    x, tgt, src, n_tgt = _cpu_case(3, ties=False)
    out = segment_sum(x, tgt, src, n_tgt, sorted_by_target=False)
    ref = torch.zeros(n_tgt, x.size(1), dtype=x.dtype)
    for e in range(tgt.numel()):
        ref[tgt[e]] += x[src[e]]
    assert torch.allclose(out, ref, rtol=1e-13, atol=1e-13)
    assert torch.equal(out, segment_weighted_sum(x, tgt, src, n_tgt,
                                                 sorted_by_target=False))


# --------------------------------------------------------------------------
# CPU: SAGEConv / GraphSAGE
# --------------------------------------------------------------------------
def _brute_agg(x_src, tgt, src, n, aggr):
    if aggr in ("max", "min"):
        return _loop(x_src, tgt, src, n, aggr == "max")[0]
    agg = torch.zeros(n, x_src.size(1), dtype=x_src.dtype)
    for e in range(tgt.numel()):
        agg[tgt[e]] += x_src[src[e]]
    if aggr == "mean":
        deg = torch.bincount(tgt, minlength=n).clamp(min=1)
        agg = agg / deg.unsqueeze(1).to(agg.dtype)
    return agg


def _conv_case(seed=4):
    g = torch.Generator().manual_seed(seed)
    n, nt, E = 14, 6, 30
    tgt = torch.randint(0, nt - 1, (E,), generator=g)  # target nt-1 empty
    src = torch.randint(0, n, (E,), generator=g)
    x = torch.randn(n, 4, generator=g, dtype=torch.float64)
    return x, torch.stack([tgt, src]), nt


def test_sageconv_aggr_argument():
    with pytest.raises(ValueError):
        SAGEConv(4, 3, aggr="bogus")
    with pytest.raises(ValueError):
        GraphSAGE(4, 3, 2, aggr="bogus")
    for rw in (True, False):
        base = SAGEConv(4, 3, root_weight=rw)
        assert base.aggr == "mean"
        keys = {k: v.shape for k, v in base.state_dict().items()}
        for aggr in ("mean", "max", "min", "sum"):
            sd = SAGEConv(4, 3, root_weight=rw, aggr=aggr).state_dict()
            assert {k: v.shape for k, v in sd.items()} == keys


def test_sageconv_default_is_the_mean_formula():
    x, ei, nt = _conv_case()
    x = x.float()
    torch.manual_seed(5)
    conv = SAGEConv(4, 3)
    tgt, src = ei[0], ei[1]
    agg = x.new_zeros(nt, 4)
    agg.index_add_(0, tgt, x.index_select(0, src))
    agg = agg / torch.bincount(tgt, minlength=nt).clamp_(min=1) \
        .unsqueeze(1).to(x.dtype)
    ref = conv.lin(torch.cat([agg, x[:nt]], dim=1))
    assert torch.equal(conv(x, ei, nt), ref)
    torch.manual_seed(5)
    assert torch.equal(SAGEConv(4, 3, aggr="mean")(x, ei, nt), ref)


@pytest.mark.parametrize("aggr", ["max", "min", "sum"])
@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("bipartite", [False, True])
def test_sageconv_aggr_matches_brute_force(aggr, root_weight, bipartite):
    x, ei, nt = _conv_case(6)
    torch.manual_seed(7)
    conv = SAGEConv(4, 3, root_weight=root_weight, aggr=aggr).double()
    if bipartite:
        g = torch.Generator().manual_seed(8)
        x_tgt = torch.randn(nt, 4, generator=g, dtype=torch.float64)
        inp, x_root = (x_tgt, x), x_tgt
    else:
        inp, x_root = x, x[:nt]
    agg = _brute_agg(x, ei[0], ei[1], nt, aggr)
    xin = torch.cat([agg, x_root], dim=1) if root_weight else agg
    ref = conv.lin(xin)
    for sbt in (False, True):   # the CPU never takes the kernels
        out = conv(inp, ei, nt, sorted_by_target=sbt)
        assert out.shape == (nt, 3)
        assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)
    if not bipartite:
        assert torch.equal(conv(x, ei, nt, fuse_relu=True),
                           torch.relu(conv(x, ei, nt)))


def test_rgnn_sage_aggr_reaches_the_convs():
    from glt_amd.models import RGNN

    et = [("a", "to", "b"), ("b", "rev", "a")]
    m = RGNN(et, 4, 8, 3, model="rsage", sage_aggr="max")
    convs = [c for layer in m.layers for c in layer.convs.values()]
    assert convs and all(c.aggr == "max" for c in convs)
    d = RGNN(et, 4, 8, 3, model="rsage")
    assert all(c.aggr == "mean" for layer in d.layers
               for c in layer.convs.values())
    assert {k: v.shape for k, v in m.state_dict().items()} == \
        {k: v.shape for k, v in d.state_dict().items()}


def test_graphsage_max_on_loader_batch(ring_graph):
    glt_amd.seed_everything(9)
    n = ring_graph["num_nodes"]
    ds = Dataset()
    ds.init_graph(edge_index=ring_graph["edge_index"], graph_mode="CPU",
                  num_nodes=n)
    ds.init_node_features(ring_graph["feats"], with_gpu=False)
    ds.init_node_labels(ring_graph["labels"])
    loader = NeighborLoader(ds, [2, 2], input_nodes=torch.arange(n),
                            batch_size=5, shuffle=True)
    data = next(iter(loader))
    torch.manual_seed(10)
    model = GraphSAGE(16, 8, 2, out_channels=n, aggr="max")
    assert all(c.aggr == "max" for c in model.convs)
    x = data.x / n
    out = model(x, data.edge_index, data.num_sampled_nodes,
                data.num_sampled_edges)
    nsn = [int(v) for v in data.num_sampled_nodes]
    nse = [int(v) for v in data.num_sampled_edges]
    assert out.shape == (nsn[0], n)
    # layer by layer with the brute-force aggregate
    h = x[:sum(nsn[:3])]
    for li, (ne, no) in enumerate(((sum(nse[:2]), sum(nsn[:2])),
                                   (nse[0], nsn[0]))):
        ei = data.edge_index[:, :ne]
        agg = _brute_agg(h, ei[0], ei[1], no, "max")
        h = model.convs[li].lin(torch.cat([agg, h[:no]], dim=1))
        if li == 0:
            h = torch.relu(h)
    assert torch.allclose(out, h, rtol=1e-5, atol=1e-6)
    loss = torch.nn.functional.cross_entropy(
        out[:data.batch_size], data.y[:data.batch_size])
    loss.backward()
    assert torch.isfinite(loss)
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()


# --------------------------------------------------------------------------
# GPU: kernels against the fp64 composition
# --------------------------------------------------------------------------
def _wide(shape, gen):
    """Magnitudes spread over four decades."""
    mag = 10.0 ** (-4.0 * torch.rand(shape, generator=gen))
    return torch.randn(shape, generator=gen) * mag


_graph_cache = {}


def _graph(n_tgt=37, n_src=50, degs=(0, 1, 3, 8, 9, 17, 70), seed=20):
    """Empty segments, full batches of 8, partial tails and a hub that
    spans many batches.  CPU tensors, built once."""
    key = (n_tgt, n_src, degs, seed)
    if key not in _graph_cache:
        g = torch.Generator().manual_seed(seed)
        deg = torch.tensor([degs[i % len(degs)] for i in range(n_tgt)])
        tgt = torch.repeat_interleave(torch.arange(n_tgt), deg)
        src = torch.randint(0, n_src, (tgt.numel(),), generator=g)
        _graph_cache[key] = (tgt, src, n_tgt, n_src)
    return _graph_cache[key]


def _values(kind, n_src, F, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "wide":
        x = _wide((n_src, F), g)
    elif kind == "ties":
        x = torch.randint(-1, 2, (n_src, F), generator=g).float()
    elif kind == "negative":
        x = -(torch.rand(n_src, F, generator=g) + 0.5)
    else:
        x = torch.rand(n_src, F, generator=g) + 0.5
    return x.to(dtype)


def _reference(x, tgt, src, n_tgt, is_max, cat, dy=None):
    """The CPU composition in fp64 on the same (CPU) inputs: (out cast to
    x's dtype, arg, fp64 dx or None)."""
    from glt_amd.ops.segment import _segment_ext_arg

    xd = x.double().requires_grad_(dy is not None)
    out = _op(is_max, cat)(xd, tgt, src, n_tgt, sorted_by_target=False)
    arg = _segment_ext_arg(x.double(), tgt, src, n_tgt, is_max)
    dx = None
    if dy is not None:
        out.backward(dy.double())
        dx = xd.grad
    return out.detach().to(x.dtype), arg, dx


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _raw_fwd(x, tgt, src, n_tgt, is_max, cat, need_arg=True):
    from glt_amd import _C
    from glt_amd.ops.segment import _offsets

    return _C.segment_ext_fwd(x, src, _offsets(tgt, n_tgt), n_tgt, is_max,
                              cat, need_arg)


def _check_forward(x, tgt, src, n_tgt):
    dev = torch.device("cuda")
    xg, tg, sg = x.to(dev), tgt.to(dev), src.to(dev)
    F = x.size(1)
    for is_max, cat in VARIANTS:
        ref, rarg, _ = _reference(x, tgt, src, n_tgt, is_max, cat)
        out, arg = _raw_fwd(xg, tg, sg, n_tgt, is_max, cat)
        assert out.dtype == x.dtype and out.shape == ref.shape
        assert arg.dtype == torch.int32 and arg.shape == (n_tgt, F)
        assert torch.equal(arg.cpu().long(), rarg), (is_max, cat)
        assert torch.equal(_bits(out), _bits(ref)), (is_max, cat)
        # the public op is the same kernel
        assert torch.equal(_bits(_op(is_max, cat)(xg, tg, sg, n_tgt)),
                           _bits(ref))


FWD_SHAPES = [(torch.float32, F) for F in (1, 64, 65, 128, 129, 256, 257)] \
    + [(torch.bfloat16, F) for F in (2, 100, 128, 130, 256)] \
    + [(torch.bfloat16, F) for F in (1, 63, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wide", "ties"])
@pytest.mark.parametrize("dtype,F", FWD_SHAPES)
def test_forward_bit_exact(dtype, F, kind):
    tgt, src, n_tgt, n_src = _graph()
    _check_forward(_values(kind, n_src, F, dtype, 30 + F), tgt, src, n_tgt)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["negative", "positive"])
@pytest.mark.parametrize("dtype,F", [(torch.float32, 129),
                                     (torch.bfloat16, 130),
                                     (torch.bfloat16, 63)])
def test_forward_one_signed_values(dtype, F, kind):
    """All-negative x under max / all-positive x under min: an accumulator
    that starts from zero would win."""
    tgt, src, n_tgt, n_src = _graph()
    x = _values(kind, n_src, F, dtype, 40 + F)
    _check_forward(x, tgt, src, n_tgt)
    out, _ = _raw_fwd(x.cuda(), tgt.cuda(), src.cuda(), n_tgt,
                      kind == "negative", False)
    nonempty = (torch.bincount(tgt, minlength=n_tgt) > 0).cuda()
    assert (out[nonempty] != 0).all() and not out[~nonempty].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F", [(torch.float32, 6),
                                     (torch.bfloat16, 6),
                                     (torch.bfloat16, 5)])
def test_forward_nan_and_infinities(dtype, F):
    tgt, src, n_tgt, n_src = _graph()
    g = torch.Generator().manual_seed(50)
    x = _values("ties", n_src, F, dtype, 51)
    x[torch.rand(n_src, F, generator=g) < 0.1] = float("nan")
    x[torch.rand(n_src, F, generator=g) < 0.2] = float("-inf")
    x[torch.rand(n_src, F, generator=g) < 0.1] = float("inf")
    for is_max, cat in VARIANTS:
        ref, rarg, _ = _reference(x, tgt, src, n_tgt, is_max, cat)
        out, arg = _raw_fwd(x.cuda(), tgt.cuda(), src.cuda(), n_tgt,
                            is_max, cat)
        out = out.cpu()
        assert torch.equal(arg.cpu().long(), rarg)
        assert torch.equal(out.isnan(), ref.isnan()) and ref.isnan().any()
        assert torch.equal(out.nan_to_num(nan=9.0), ref.nan_to_num(nan=9.0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forward_grid_stride(dtype):
    """More targets than the 8192 waves of the grid."""
    n_tgt = 3 * 8192 + 5
    tgt, src, _, n_src = _graph(n_tgt, n_tgt + 7, (0, 1, 2), 21)
    x = _values("ties", n_src, 2, dtype, 60)
    dev = torch.device("cuda")
    for is_max, cat in ((True, False), (False, True)):
        ref, rarg, _ = _reference(x, tgt, src, n_tgt, is_max, cat)
        out, arg = _raw_fwd(x.to(dev), tgt.to(dev), src.to(dev), n_tgt,
                            is_max, cat)
        assert torch.equal(arg.cpu().long(), rarg)
        assert torch.equal(_bits(out), _bits(ref))


def _gpu_grad(x, tgt, src, n_tgt, is_max, cat, dy):
    dev = torch.device("cuda")
    xg = x.to(dev).requires_grad_(True)
    out = _op(is_max, cat)(xg, tgt.to(dev), src.to(dev), n_tgt)
    out.backward(dy.to(dev))
    assert xg.grad.dtype == x.dtype and xg.grad.shape == x.shape
    return xg.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F", [1, 65, 130])
def test_backward_exact_on_integers(dtype, F):
    from glt_amd.ops import is_deterministic, set_deterministic

    tgt, src, n_tgt, n_src = _graph()
    x = _values("ties", n_src, F, dtype, 70 + F)
    g = torch.Generator().manual_seed(71 + F)
    for is_max, cat in VARIANTS:
        w = 2 * F if cat else F
        dy = torch.randint(-4, 5, (n_tgt, w), generator=g).to(dtype)
        dy[0, 0] = 4
        _, _, rdx = _reference(x, tgt, src, n_tgt, is_max, cat, dy)
        _, _, mag = _reference(x, tgt, src, n_tgt, is_max, cat, dy.abs())
        # deterministic mode: max|dy| = 4 puts the grid at 2^-15 and the
        # exact-sum headroom at 2^6 * 2^3 = 512
        assert dy.abs().max() == 4 and mag.max() < 2 ** H * 8
        ref = rdx.to(dtype)          # the exact value, rounded once
        assert not is_deterministic()
        assert torch.equal(_bits(_gpu_grad(x, tgt, src, n_tgt, is_max, cat,
                                           dy)), _bits(ref))
        set_deterministic(True)
        try:
            det = _gpu_grad(x, tgt, src, n_tgt, is_max, cat, dy)
        finally:
            set_deterministic(False)
        assert torch.equal(_bits(det), _bits(ref))


def _low_precision(bound, ref, dtype):
    if dtype == torch.bfloat16:
        return UBF * (ref.abs() + bound) + bound
    return bound


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("F", [7, 130])
def test_backward_general_values(dtype, F):
    from glt_amd.ops import set_deterministic

    tgt, src, n_tgt, n_src = _graph()
    x = _values("ties", n_src, F, dtype, 80 + F)   # ties: shared winners
    g = torch.Generator().manual_seed(81 + F)
    for is_max, cat in VARIANTS:
        w = 2 * F if cat else F
        dy = _wide((n_tgt, w), g).to(dtype)
        _, rarg, rdx = _reference(x, tgt, src, n_tgt, is_max, cat, dy)
        _, _, mag = _reference(x, tgt, src, n_tgt, is_max, cat, dy.abs())
        cnt = torch.zeros(n_src, F, dtype=torch.float64)
        cnt.scatter_add_(0, rarg.clamp(min=0), (rarg >= 0).double())
        if cat:
            cnt[:n_tgt] += 1
        assert cnt.max() > 2 and cnt.max() <= 2 ** H
        bound = _low_precision((cnt - 1).clamp(min=0) * U24 * mag, rdx,
                               dtype)
        err = (_gpu_grad(x, tgt, src, n_tgt, is_max, cat, dy).double()
               - rdx).abs()
        print("plain %s F=%d max=%s cat=%s: max err %.3e, max bound %.3e" % (
            dtype, F, is_max, cat, err.max().item(), bound.max().item()))
        assert (err <= bound).all()

        set_deterministic(True)
        try:
            runs = [_gpu_grad(x, tgt, src, n_tgt, is_max, cat, dy)
                    for _ in range(2)]
        finally:
            set_deterministic(False)
        assert torch.equal(_bits(runs[0]), _bits(runs[1]))
        B = dy.double().abs().max().item()
        e = math.frexp(B)[1]             # 2^(e-1) <= B < 2^e
        q = 2.0 ** (e + H - 24)
        bound = _low_precision(cnt * (q / 2 + U24 * B), rdx, dtype)
        err = (runs[0].double() - rdx).abs()
        print("det   %s F=%d max=%s cat=%s: max err %.3e, max bound %.3e" % (
            dtype, F, is_max, cat, err.max().item(), bound.max().item()))
        assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,F", [(torch.float32, 70),
                                     (torch.bfloat16, 70),
                                     (torch.bfloat16, 9)])
def test_need_arg(dtype, F):
    from glt_amd.ops import segment_max_cat

    tgt, src, n_tgt, n_src = _graph()
    dev = torch.device("cuda")
    x = _values("ties", n_src, F, dtype, 90).to(dev)
    tg, sg = tgt.to(dev), src.to(dev)
    for is_max, cat in VARIANTS:
        out, arg = _raw_fwd(x, tg, sg, n_tgt, is_max, cat, need_arg=True)
        out2, none = _raw_fwd(x, tg, sg, n_tgt, is_max, cat, need_arg=False)
        assert none is None and arg is not None
        assert torch.equal(_bits(out), _bits(out2))
    xx = x.clone().requires_grad_(True)
    with_grad = segment_max_cat(xx, tg, sg, n_tgt)
    assert with_grad.requires_grad
    with torch.no_grad():
        without = segment_max_cat(xx, tg, sg, n_tgt)
    assert not without.requires_grad
    assert torch.equal(_bits(with_grad.detach()), _bits(without))
    assert torch.equal(_bits(segment_max_cat(x, tg, sg, n_tgt)),
                       _bits(without))


@pytest.mark.gpu
def test_validation_and_empty_shapes():
    from glt_amd import _C
    from glt_amd.ops.segment import _offsets

    tgt, src, n_tgt, n_src = _graph()
    dev = torch.device("cuda")
    F = 6
    x = _values("ties", n_src, F, torch.float32, 95).to(dev)
    tg, sg = tgt.to(dev), src.to(dev)
    off = _offsets(tg, n_tgt)
    dy = torch.ones(n_tgt, F, device=dev)
    dy2 = torch.ones(n_tgt, 2 * F, device=dev)

    def valid():
        out, arg = _C.segment_ext_fwd(x, sg, off, n_tgt, True, True, True)
        dx = _C.segment_ext_bwd(dy2, arg, n_src, True, False)
        torch.cuda.synchronize()
        assert out.shape == (n_tgt, 2 * F) and dx.shape == (n_src, F)
        assert dx.dtype == torch.float32
        return arg

    arg = valid()
    wide = torch.zeros(n_src, 2 * F, device=dev)
    bad = [
        lambda: _C.segment_ext_fwd(x, sg.int(), off, n_tgt, True, False,
                                   True),
        lambda: _C.segment_ext_fwd(wide[:, ::2], sg, off, n_tgt, True,
                                   False, True),
        lambda: _C.segment_ext_fwd(x, sg, off[:-1], n_tgt, True, False,
                                   True),
        lambda: _C.segment_ext_fwd(x, sg, off, n_tgt + 1, True, False, True),
        lambda: _C.segment_ext_fwd(x.half(), sg, off, n_tgt, True, False,
                                   True),
        lambda: _C.segment_ext_fwd(x[:n_tgt - 1].contiguous(), sg, off,
                                   n_tgt, True, True, True),
        lambda: _C.segment_ext_bwd(dy, arg.long(), n_src, False, False),
        lambda: _C.segment_ext_bwd(dy, arg[:, :F - 1].contiguous(), n_src,
                                   False, False),
        lambda: _C.segment_ext_bwd(dy, arg[:-1], n_src, False, False),
        lambda: _C.segment_ext_bwd(dy, arg.cpu(), n_src, False, False),
        lambda: _C.segment_ext_bwd(dy2[:, :2 * F - 1], arg, n_src, True,
                                   False),
        lambda: _C.segment_ext_bwd(dy2, arg, n_tgt - 1, True, False),
        lambda: _C.segment_ext_bwd(dy.half(), arg, n_src, False, False),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail("case %d did not raise" % i)
        valid()

    # F == 0 and n_tgt == 0: the right empty shapes, no launch
    x0 = torch.zeros(n_src, 0, device=dev)
    for cat in (False, True):
        out, a = _C.segment_ext_fwd(x0, sg, off, n_tgt, True, cat, True)
        assert out.shape == (n_tgt, 0) and a.shape == (n_tgt, 0)
        assert a.dtype == torch.int32
        dx = _C.segment_ext_bwd(out, a, n_src, cat, False)
        assert dx.shape == (n_src, 0)
        none = torch.zeros(0, dtype=torch.long, device=dev)
        off0 = torch.zeros(1, dtype=torch.long, device=dev)
        out, a = _C.segment_ext_fwd(x, none, off0, 0, False, cat, True)
        assert out.shape == (0, 2 * F if cat else F) and a.shape == (0, F)
        dx = _C.segment_ext_bwd(out, a, n_src, cat, True)
        assert dx.shape == (n_src, F) and not dx.any()
    valid()


# --------------------------------------------------------------------------
# GPU: layer and model
# --------------------------------------------------------------------------
def _within_twice(name, fused, comp, ref):
    ef = (fused.double().cpu() - ref).abs().max().item()
    ec = (comp.double().cpu() - ref).abs().max().item()
    print("%s: fused err %.3e, composite err %.3e" % (name, ef, ec))
    assert ef <= 2 * ec + 1e-6 * ref.abs().max().item(), name


def _run_layer(conv, x, ei, nt, gy, **kw):
    """out, dx, dW and the aggregate handed to the projection."""
    seen = {}
    project = conv._project

    def spy(xin, fuse_relu):
        seen["xin"] = xin.detach()
        return project(xin, fuse_relu)

    conv.zero_grad()
    conv._project = spy
    try:
        xx = x.clone().requires_grad_(True)
        out = conv(xx, ei, nt, **kw)
    finally:
        del conv._project
    out.backward(gy.to(out.dtype))
    return {"out": out.detach(), "dx": xx.grad,
            "dW": conv.lin.weight.grad.clone()}, seen["xin"]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("root_weight", [True, False])
def test_sageconv_max_fused_vs_fallback_vs_fp64(root_weight, dtype):
    g = torch.Generator().manual_seed(100)
    n, nt = 300, 120
    deg = torch.randint(0, 13, (nt,), generator=g)
    tgt = torch.repeat_interleave(torch.arange(nt), deg)
    src = torch.randint(0, n, (tgt.numel(),), generator=g)
    ei = torch.stack([tgt, src])
    x = torch.randn(n, 16, generator=g).to(dtype)
    gy = torch.randn(nt, 8, generator=g)
    torch.manual_seed(101)
    conv = SAGEConv(16, 8, root_weight=root_weight, aggr="max")
    ref, _ = _run_layer(copy.deepcopy(conv).double(), x.double(), ei, nt,
                        gy.double())
    conv = conv.cuda()
    args = (x.cuda(), ei.cuda(), nt, gy.cuda())
    fused, xin_f = _run_layer(conv, *args, sorted_by_target=True)
    comp, xin_c = _run_layer(conv, *args, sorted_by_target=False)
    assert xin_f.dtype == dtype
    assert xin_f.shape == (nt, 32 if root_weight else 16)
    assert torch.equal(_bits(xin_f), _bits(xin_c))
    for k in ref:
        _within_twice(k, fused[k], comp[k], ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("aggr", ["max", "min"])
def test_graphsage_aggr_on_gpu_loader_batch(aggr):
    dev = torch.device("cuda", 0)
    glt_amd.seed_everything(110)
    g = torch.Generator().manual_seed(110)
    n, E = 2000, 16000
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack(
        [torch.randint(0, n, (E,), generator=g),
         torch.randint(0, n, (E,), generator=g)]), graph_mode="CUDA",
        num_nodes=n, device=0)
    ds.init_node_features(torch.randn(n, 32, generator=g), split_ratio=1.0,
                          device=0)
    ds.init_node_labels(torch.randint(0, 5, (n,), generator=g))
    loader = NeighborLoader(ds, [5, 5], input_nodes=torch.arange(256),
                            batch_size=128, device=dev, to_device=dev)
    data = next(iter(loader))
    model = GraphSAGE(32, 16, 2, out_channels=5, aggr=aggr).to(dev)
    trims = (data.num_sampled_nodes, data.num_sampled_edges)
    bs = data.batch_size
    out = model(data.x, data.edge_index, *trims)[:bs]
    loss = torch.nn.functional.cross_entropy(out, data.y[:bs])
    loss.backward()
    assert torch.isfinite(loss)
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    # same batch and weights on the CPU: fp64 is the reference, the fp32
    # composition the yardstick
    cpu = copy.deepcopy(model).cpu()
    xc, eic = data.x.cpu(), data.edge_index.cpu()
    with torch.no_grad():
        comp = cpu(xc, eic, *trims)[:bs]
        ref = cpu.double()(xc.double(), eic, *trims)[:bs]
    _within_twice("logits " + aggr, out.detach(), comp, ref)

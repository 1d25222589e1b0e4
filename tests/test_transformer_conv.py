"""Dot-product attention with edge features: ops.transformer_attention, the
hip_tconv kernels, TransformerConv and GraphTransformer.

Edges (t = tgt[e], s = src[e]):

    kk_e       = k[s] + ee[e],  vv_e = v[s] + ee[e]     (ee absent: k, v)
    score_e[h] = scale * <q[t,h,:], kk_e[h,:]>
    p_e[h]     = softmax over seg(t) of score_e[h]
    out[t,h,:] = sum_{e in seg(t)} p_e[h] * vv_e[h,:]   (empty: 0)
    ds_e       = p_e * (<dout_t, vv_e> - <dout_t, out_t>)
    dq[t]      = scale * sum_{e in seg(t)} ds_e * kk_e
    dk[s]      = scale * sum_{e: src[e]=s} ds_e * q[t_e]
    dv[s]      =         sum_{e: src[e]=s} p_e * dout[t_e]
    dee[e]     = scale * ds_e * q[t] + p_e * dout[t]

The reference of every GPU test is `_ref64`: these lines in fp64 on the CPU
from the exact inputs (for bf16, the bf16-rounded inputs), gradients from
the written formulas, not from autograd.

Bounds, the project's own (tests/test_gatv2.py); nothing is tuned to what
the kernels give.
  fp32, "rule 3": the fused path's max error against fp64 is at most twice
    the max error of the torch composition run in fp32 on the same GPU,
    plus 1e-6 * max|ref|.
  bf16: |x - ref| <= 2^-8 |ref| + b32, b32 = the max error of the fp32 fused
    run on the same bf16-rounded inputs: all math is fp32 and every result
    is rounded once (RNE, 2^-9 relative).
  exact tests: bit equality, argued in their docstrings.
"""
import copy
import math

import pytest
import torch

import glt_amd
from glt_amd import Dataset, NeighborLoader
from glt_amd.models import GraphTransformer, TransformerConv
from glt_amd.ops import (transformer_attention,
                         transformer_attention_composition,
                         transformer_attention_fused_ok)

UBF = 2.0 ** -8
KEYS = ("out", "dq", "dk", "dv", "dee")
# in-degrees: an empty segment, the edges of the 4-edge batch, a list longer
# than a wave has lanes, and two targets of in-degree 1
DEGS = (0, 1, 4, 5, 9, 70, 1, 3)
SHAPES = [(1, 1), (3, 4), (4, 64), (2, 128), (5, 64), (2, 20), (1, 65)]


def _ref64(q, k, v, ee, tgt, src, n_tgt, scale, dout):
    q, k, v, dout = (x.detach().double().cpu() for x in (q, k, v, dout))
    tgt, src = tgt.cpu(), src.cpu()
    H = k.size(1)
    kk, vv = k[src], v[src]
    if ee is not None:
        ee = ee.detach().double().cpu()
        kk, vv = kk + ee, vv + ee
    score = scale * (q[tgt] * kk).sum(-1)
    m = torch.full((n_tgt, H), float("-inf"), dtype=torch.float64)
    m.scatter_reduce_(0, tgt.unsqueeze(1).expand_as(score), score,
                      reduce="amax")
    ex = (score - m[tgt]).exp()
    p = ex / torch.zeros(n_tgt, H, dtype=torch.float64).index_add_(
        0, tgt, ex)[tgt]
    out = torch.zeros(n_tgt, H, k.size(2), dtype=torch.float64)
    out.index_add_(0, tgt, p.unsqueeze(-1) * vv)
    ds = (p * ((dout[tgt] * vv).sum(-1) - (dout * out).sum(-1)[tgt]))
    ds, p = ds.unsqueeze(-1), p.unsqueeze(-1)
    res = dict(
        out=out, score=score,
        dq=torch.zeros_like(q).index_add_(0, tgt, scale * ds * kk),
        dk=torch.zeros_like(k).index_add_(0, src, scale * ds * q[tgt]),
        dv=torch.zeros_like(v).index_add_(0, src, p * dout[tgt]))
    if ee is not None:
        res["dee"] = scale * ds * q[tgt] + p * dout[tgt]
    return res


def _run(fn, q, k, v, ee, tgt, src, n_tgt, scale, dout, grads="qkve"):
    ins = dict(q=q, k=k, v=v, e=ee)
    ins = {n: None if x is None else
           x.detach().clone().requires_grad_(n in grads)
           for n, x in ins.items()}
    out = fn(ins["q"], ins["k"], ins["v"], tgt, src, n_tgt, edge=ins["e"],
             scale=scale)
    out.backward(dout.to(out.dtype))
    res = dict(out=out.detach(), dq=ins["q"].grad, dk=ins["k"].grad,
               dv=ins["v"].grad)
    if ee is not None:
        res["dee"] = ins["e"].grad
    return res


def _max_err(x, ref):
    return (x.double().cpu() - ref).abs().max().item() if ref.numel() else 0.


def _within_twice(name, fused, comp, ref, check=True):
    ef, ec = _max_err(fused, ref), _max_err(comp, ref)
    scale = ref.abs().max().item() if ref.numel() else 0.
    print("%s: fused err %.3e, composition err %.3e, max|ref| %.3e" % (
        name, ef, ec, scale))
    if check:
        assert ef <= 2 * ec + 1e-6 * scale, name


def _case(H, C, with_ee, seed=0, degs=DEGS, n_src=90, dev="cuda"):
    """(q, k, v, ee, tgt, src, n_tgt, scale, dout) in fp32.  Sources 80..89
    have no edge, source 3 is hit by every target that has one; q has one
    row more than there are targets."""
    g = torch.Generator().manual_seed(seed)
    n_tgt = len(degs)
    tgt = torch.repeat_interleave(torch.arange(n_tgt), torch.tensor(degs))
    E = tgt.numel()
    src = torch.randint(0, 80, (E,), generator=g)
    src[torch.tensor(degs).cumsum(0)[torch.tensor(degs) > 0] - 1] = 3
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    return (rnd(n_tgt + 1, H, C), rnd(n_src, H, C), rnd(n_src, H, C),
            rnd(E, H, C) if with_ee else None, tgt.to(dev), src.to(dev),
            n_tgt, 1.0 / math.sqrt(C), rnd(n_tgt, H, C))


def _check_fp32_and_bf16(case, views=lambda q, k, v: (q, k, v)):
    """Rule 3 in fp32, then the bf16 bound, on one case."""
    q, k, v, ee, tgt, src, n_tgt, scale, dout = case
    for dtype in (torch.float32, torch.bfloat16):
        r = [None if x is None else x.to(dtype).float()
             for x in (q, k, v, ee, dout)]
        rest = (tgt, src, n_tgt, scale)
        ref = _ref64(r[0], r[1], r[2], r[3], *rest, r[4])
        f32 = _run(transformer_attention, *views(*r[:3]), r[3], *rest, r[4])
        if dtype == torch.float32:
            comp = _run(transformer_attention_composition, *r[:4], *rest,
                        r[4])
            for key in f32:
                assert f32[key].shape == ref[key].shape, key
                _within_twice(key, f32[key], comp[key], ref[key])
            continue
        low = [None if x is None else x.to(dtype) for x in r]
        b16 = _run(transformer_attention, *views(*low[:3]), low[3], *rest,
                   low[4])
        for key in b16:
            assert b16[key].dtype == dtype, key
            err = (b16[key].double().cpu() - ref[key]).abs()
            bound = UBF * ref[key].abs() + _max_err(f32[key], ref[key])
            print("%s bf16: max err %.3e" % (key, err.max().item()))
            assert (err <= bound).all(), key


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
@pytest.mark.parametrize("with_ee", [False, True])
def test_composition_matches_per_edge_loop(with_ee):
    """Target 2 has no edge, target 1 one edge, target 0 takes source 4
    twice; edges are not sorted."""
    g = torch.Generator().manual_seed(0)
    tgt = torch.tensor([3, 0, 1, 0, 3, 0, 3])
    src = torch.tensor([5, 4, 2, 4, 0, 1, 5])
    n_tgt, n_src, H, C, scale, E = 4, 7, 2, 3, 0.7, 7
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q, k, v, dout = rnd(n_tgt + 1, H, C), rnd(n_src, H, C), \
        rnd(n_src, H, C), rnd(n_tgt, H, C)
    ee = rnd(E, H, C) if with_ee else None
    assert not transformer_attention_fused_ok(q, k, v, ee)
    got = _run(transformer_attention, q, k, v, ee, tgt, src, n_tgt, scale,
               dout)
    zero = torch.zeros(H, C, dtype=torch.float64)
    want = dict(out=torch.zeros_like(dout), dq=torch.zeros_like(q),
                dk=torch.zeros_like(k), dv=torch.zeros_like(v),
                dee=torch.zeros(E, H, C, dtype=torch.float64))
    for h in range(H):
        kk = [k[src[e], h] + (ee[e, h] if with_ee else zero[h])
              for e in range(E)]
        vv = [v[src[e], h] + (ee[e, h] if with_ee else zero[h])
              for e in range(E)]
        sc = [scale * (q[tgt[e], h] @ kk[e]) for e in range(E)]
        p = [0.0] * E
        for t in range(n_tgt):
            seg = [e for e in range(E) if tgt[e] == t]
            z = sum(torch.exp(sc[e]) for e in seg)
            for e in seg:
                p[e] = torch.exp(sc[e]) / z
                want["out"][t, h] += p[e] * vv[e]
        for e in range(E):
            t, s = tgt[e], src[e]
            ds = p[e] * (dout[t, h] @ vv[e] - dout[t, h] @ want["out"][t, h])
            want["dq"][t, h] += scale * ds * kk[e]
            want["dk"][s, h] += scale * ds * q[t, h]
            want["dv"][s, h] += p[e] * dout[t, h]
            want["dee"][e, h] = scale * ds * q[t, h] + p[e] * dout[t, h]
    ref = _ref64(q, k, v, ee, tgt, src, n_tgt, scale, dout)
    for key in got:
        assert torch.allclose(got[key], want[key], rtol=1e-11, atol=1e-12)
        assert torch.allclose(ref[key], want[key], rtol=1e-11, atol=1e-12)
    assert not got["out"][2].any() and not got["dq"][[2, 4]].any()
    assert not got["dk"][[3, 6]].any()        # sources without an edge
    o16 = transformer_attention_composition(
        q.bfloat16(), k.bfloat16(), v.bfloat16(), tgt, src, n_tgt,
        None if ee is None else ee.bfloat16(), scale)
    assert o16.dtype == torch.bfloat16
    assert torch.allclose(o16.double(), want["out"], atol=0.1)


def test_layer_loads_pyg_state_dict():
    conv = TransformerConv(8, 4, heads=3, beta=True, edge_dim=5)
    names = {"lin_key.weight", "lin_key.bias", "lin_query.weight",
             "lin_query.bias", "lin_value.weight", "lin_value.bias",
             "lin_edge.weight", "lin_skip.weight", "lin_skip.bias",
             "lin_beta.weight"}
    shapes = {n: (12, 8) for n in names if n.endswith("weight")}
    shapes.update({n: (12,) for n in names if n.endswith("bias")})
    shapes.update({"lin_edge.weight": (12, 5), "lin_beta.weight": (1, 36)})
    g = torch.Generator().manual_seed(1)
    sd = {n: torch.randn(*s, generator=g) for n, s in shapes.items()}
    conv.load_state_dict(sd)                  # strict
    assert set(conv.state_dict()) == names and conv.use_fused
    mean = TransformerConv(8, 4, heads=3, concat=False, root_weight=False)
    assert set(mean.state_dict()) == {n for n in names if n[4] in "kqv"}
    x = torch.randn(6, 8, generator=g)
    ei = torch.tensor([[0, 0, 1, 3], [5, 2, 2, 4]])
    assert conv(x, ei, torch.randn(4, 5, generator=g), 4).shape == (4, 12)
    assert mean(x, ei, num_target=4).shape == (4, 4)
    with pytest.raises(ValueError):
        conv(x, ei, None, 4)


def test_graph_transformer_trains_on_edge_batch(ring_graph):
    n = ring_graph["num_nodes"]
    ds = Dataset()
    ds.init_graph(edge_index=ring_graph["edge_index"], graph_mode="CPU",
                  num_nodes=n)
    ds.init_node_features(ring_graph["feats"], with_gpu=False)
    ds.init_edge_features(ring_graph["efeats"], with_gpu=False)
    ds.init_node_labels(ring_graph["labels"])
    data = next(iter(NeighborLoader(ds, [2, 2], input_nodes=torch.arange(n),
                                    batch_size=5, with_edge=True)))
    assert data.edge_attr.size(0) == data.edge_index.size(1)
    torch.manual_seed(2)
    model = GraphTransformer(data.x.size(1), 8, int(data.y.max()) + 1, 2,
                             heads=2, edge_dim=data.edge_attr.size(1))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = copy.deepcopy(model.state_dict())
    out = model(data.x.float(), data.edge_index, data.num_sampled_nodes,
                data.num_sampled_edges, data.edge_attr.float())
    loss = torch.nn.functional.cross_entropy(out[:data.batch_size],
                                             data.y[:data.batch_size])
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    assert all(not torch.equal(v, before[n])
               for n, v in model.state_dict().items() if "weight" in n)


# --------------------------------------------------------------------------
# GPU: kernels against fp64
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_ee", [False, True])
@pytest.mark.parametrize("H,C", SHAPES)
def test_fused_against_fp64(H, C, with_ee):
    case = _case(H, C, with_ee)
    assert transformer_attention_fused_ok(*case[:4])
    _check_fp32_and_bf16(case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["kv_slices", "q_off_by_one"])
def test_fused_on_views(kind):
    """k and v as column slices of one [n_src, 2*H*C] projection are read
    in place; a q whose base is one element off the wide alignment takes
    the row layout and still agrees."""
    def views(q, k, v):
        if kind == "kv_slices":
            kv = torch.cat([k.flatten(1), v.flatten(1)], 1)
            return q, kv[:, :256].view(-1, 4, 64), kv[:, 256:].view(-1, 4, 64)
        buf = torch.zeros(q.numel() + 1, dtype=q.dtype, device=q.device)
        buf[1:] = q.flatten()
        return buf[1:].view(q.shape), k, v
    _check_fp32_and_bf16(_case(4, 64, True, seed=3), views)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_single_edge_and_mean(dtype):
    """In-degree 1: m = score, p = exp(0) = 1, Z = 1, so out = 1 * vv_e / 1
    with vv_e = fl32(v + ee) rounded once to the dtype: bit equal to the
    same sum in torch.  q = 0: every score is 0 and p = 1 before the
    division, so out = (sum of vv_e) * (1 / deg); with small integers and
    power-of-two degrees the sum, 1 / deg and the product are exact in
    fp32 and, halves and quarters of integers below 64, in bf16."""
    q, k, v, ee, tgt, src, n_tgt, scale, _ = _case(
        4, 64, True, seed=4, degs=(1, 4, 1, 2, 8, 0))
    q, k, v, ee = (x.to(dtype) for x in (q, k, v, ee))
    out = transformer_attention(q, k, v, tgt, src, n_tgt, edge=ee)
    for t in (0, 2):
        e = int((tgt == t).nonzero())
        want = (v[src[e]].float() + ee[e].float()).to(dtype)
        assert torch.equal(out[t], want)
    g = torch.Generator().manual_seed(5)
    k, v, ee = (torch.randint(-4, 5, x.shape, generator=g).to(x) for x in
                (k, v, ee))
    out = transformer_attention(torch.zeros_like(q), k, v, tgt, src, n_tgt,
                                edge=ee)
    vv = (v[src].double() + ee.double()).cpu()
    mean = torch.zeros(n_tgt, 4, 64, dtype=torch.float64).index_add_(
        0, tgt.cpu(), vv) / torch.tensor(
            [1, 4, 1, 2, 8, 1], dtype=torch.float64).view(-1, 1, 1)
    assert torch.equal(out.double().cpu(), mean)


@pytest.mark.gpu
def test_two_runs_are_bit_identical():
    case = _case(5, 64, True, seed=6)
    for dtype in (torch.float32, torch.bfloat16):
        c = [x.to(dtype) if torch.is_tensor(x) and x.is_floating_point()
             else x for x in case]
        a = _run(transformer_attention, *c)
        b = _run(transformer_attention, *c)
        for key in a:
            assert torch.equal(a[key], b[key]), key


@pytest.mark.gpu
def test_large_scores():
    """q scaled so that |score| reaches about 100.  out is held to rule 3;
    the gradient errors of both paths are printed, not asserted."""
    q, *rest = _case(4, 64, True, seed=7)
    q = q * 40
    ref = _ref64(q, *rest)
    print("max |score| %.1f" % ref["score"].abs().max().item())
    assert ref["score"].abs().max() > 80
    fused = _run(transformer_attention, q, *rest)
    comp = _run(transformer_attention_composition, q, *rest)
    for key in fused:
        assert torch.isfinite(fused[key]).all(), key
        _within_twice(key, fused[key], comp[key], ref[key],
                      check=key == "out")


@pytest.mark.gpu
def test_gradient_subsets(monkeypatch):
    """Only q wants a gradient: dk, dv and dee are None and the by-source
    index is never built.  ee without a gradient: dee is None."""
    from glt_amd import _C

    case = _case(4, 64, True, seed=8)
    full = _run(transformer_attention, *case)
    no_e = _run(transformer_attention, *case, grads="qkv")
    assert no_e["dee"] is None
    for key in ("dq", "dk", "dv"):
        assert torch.equal(no_e[key], full[key]), key

    def boom(*a, **kw):
        raise AssertionError("by-source index built without need")
    monkeypatch.setattr(_C, "segment_transpose", boom)
    only_q = _run(transformer_attention, *case, grads="q")
    assert only_q["dk"] is None and only_q["dv"] is None \
        and only_q["dee"] is None
    assert torch.equal(only_q["dq"], full["dq"])


@pytest.mark.gpu
def test_entry_point_rejects_bad_input():
    from glt_amd import _C

    q, k, v, ee, tgt, src, n_tgt, scale, _ = _case(2, 8, True)
    off = torch.searchsorted(tgt, torch.arange(n_tgt + 1, device=tgt.device))
    _C.tconv_fwd(q, k, v, ee, src, off, n_tgt, scale)
    wide = torch.zeros(90, 2, 129, device=q.device)
    for args in [(q.double(), k, v, ee, src, off),
                 (q.bfloat16(), k, v, ee, src, off),
                 (wide[:9], wide, wide, None, src, off),
                 (q, k, v, ee, src, off[:-1]),
                 (q, k, v, ee[:-1], src, off),
                 (q.cpu(), k.cpu(), v.cpu(), None, src.cpu(), off.cpu())]:
        with pytest.raises(RuntimeError, match="tconv"):
            _C.tconv_fwd(*args, n_tgt, scale)
    out, m, z, o32 = _C.tconv_fwd(q, k, v, None, src[:0], off * 0, n_tgt,
                                  scale)
    assert not out.any() and out.shape == (n_tgt, 2, 8) and o32 is None


# --------------------------------------------------------------------------
# GPU: layer
# --------------------------------------------------------------------------
@pytest.mark.gpu
def test_layer_fused_vs_composition_vs_fp64(monkeypatch):
    """TransformerConv(edge_dim, beta=True, concat=False) on one sampled
    batch: rule 3 on the output and every parameter gradient, the fp64 copy
    on the CPU as the reference, use_fused = False as the yardstick."""
    import glt_amd.ops.attention as att_ops

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(9)
    n, E = 1500, 12000
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack([
        torch.randint(0, n, (E,), generator=g),
        torch.randint(0, n, (E,), generator=g)]), graph_mode="CUDA",
        num_nodes=n, device=0)
    ds.init_node_features(torch.randn(n, 32, generator=g), split_ratio=1.0,
                          device=0)
    ds.init_edge_features(torch.randn(E, 6, generator=g), split_ratio=1.0,
                          device=0)
    glt_amd.seed_everything(10)
    data = next(iter(NeighborLoader(ds, [6], input_nodes=torch.arange(128),
                                    batch_size=128, device=dev,
                                    to_device=dev, with_edge=True)))
    nt = data.batch_size
    torch.manual_seed(11)
    conv = TransformerConv(32, 16, heads=4, concat=False, beta=True,
                           edge_dim=6)
    gy = torch.randn(nt, 16, generator=g)
    calls = []
    real = att_ops._TconvFused.apply
    monkeypatch.setattr(att_ops._TconvFused, "apply",
                        lambda *a: calls.append(1) or real(*a))

    def run(mod, cast):
        mod.zero_grad()
        out = mod(cast(data.x), data.edge_index.to(cast(data.x).device),
                  cast(data.edge_attr), nt)
        out.backward(gy.to(out.device, out.dtype))
        res = {n: p.grad.clone() for n, p in mod.named_parameters()}
        res["out"] = out.detach()
        return res

    ref = run(copy.deepcopy(conv).double(), lambda x: x.double().cpu())
    conv = conv.to(dev)
    fused = run(conv, lambda x: x.float())
    conv.use_fused = False
    comp = run(conv, lambda x: x.float())
    assert len(calls) == 1     # the fused run took the kernels, only it
    assert set(fused) == set(ref) == set(comp) and len(ref) == 11
    for key in ref:
        _within_twice(key, fused[key], comp[key], ref[key])

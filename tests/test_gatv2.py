"""GATv2 attention: ops.gatv2_softmax_aggregate, the hip_gatv2 kernels,
GATv2Conv, GAT(v2=True) and RGNN('rgatv2').

Edges (t = tgt[e], s = src[e]), hl = source projection, hr = target
projection, att [H, C]:

    u_e[h,c]   = hl[s,h,c] + hr[t,h,c]
    score_e[h] = sum_c att[h,c] * leaky_relu(u_e[h,c], slope)
    p_e[h]     = softmax over seg(t) of score_e[h]
    out[t,h,:] = sum_{e in seg(t)} p_e[h] * hl[s,h,:]     (empty: 0)
    ds_e       = p_e * (<dout_t, hl_s> - <dout_t, out_t>)
    g_e[c]     = ds_e * att[c] * (u_e[c] > 0 ? 1 : slope)
    dhl[s]     = sum_{e: src[e]=s} (p_e * dout_t + g_e)
    dhr[t]     = sum_{e in seg(t)} g_e
    datt[h,c]  = sum_e ds_e * leaky_relu(u_e[c])

The reference of every GPU test is `_ref64`: these lines in fp64 on the
CPU from the exact inputs (for bf16, the bf16-rounded inputs), gradients
from the written formulas, not from autograd.

Bounds.  Nothing here is tuned to what the kernels give.
  fp32 ("rule 3", the yardstick rule of test_weighted_segment.py): the
    fused path's max error against fp64 is at most twice the max error of
    the torch composition run in fp32 on the GPU, plus 1e-6 * max|ref|.
  bf16 out / dhl / dhr: |x - ref| <= 2^-8 |ref| + b32, b32 = the max error
    of the fp32 fused run on the same bf16-rounded inputs: the kernels do
    all math in fp32 and round each result once (RNE, 2^-9 relative).
    datt stays fp32 and follows rule 3.
  exact tests: bit equality, argued in their docstrings.
"""
import copy

import pytest
import torch

import glt_amd
from glt_amd import Dataset, NeighborLoader
from glt_amd.models import GAT, GATConv, GATv2Conv, RGNN
from glt_amd.models.hetero import HeteroConv
from glt_amd.ops import gatv2_composition, gatv2_softmax_aggregate

UBF = 2.0 ** -8
KEYS = ("out", "dhl", "dhr", "datt")


# --------------------------------------------------------------------------
# the definition
# --------------------------------------------------------------------------
def _ref64(hr, hl, att, tgt, src, n_tgt, slope, dout):
    """dict(out, dhl, dhr, datt) in fp64 on the CPU."""
    hr, hl, att, dout = (v.detach().double().cpu()
                         for v in (hr, hl, att, dout))
    tgt, src = tgt.cpu(), src.cpu()
    H = hl.size(1)
    hs = hl[src]
    u = hs + hr[tgt]
    lr = torch.where(u > 0, u, u * slope)
    score = (lr * att).sum(-1)
    m = torch.full((n_tgt, H), float("-inf"), dtype=torch.float64)
    m.scatter_reduce_(0, tgt.unsqueeze(1).expand_as(score), score,
                      reduce="amax")
    ex = (score - m[tgt]).exp()
    p = ex / torch.zeros(n_tgt, H, dtype=torch.float64).index_add_(
        0, tgt, ex)[tgt]
    out = torch.zeros(n_tgt, H, hl.size(2), dtype=torch.float64)
    out.index_add_(0, tgt, p.unsqueeze(-1) * hs)
    ds = p * ((dout[tgt] * hs).sum(-1) - (dout * out).sum(-1)[tgt])
    g = ds.unsqueeze(-1) * att * torch.where(
        u > 0, torch.ones_like(u), torch.full_like(u, slope))
    dhl = torch.zeros_like(hl).index_add_(
        0, src, p.unsqueeze(-1) * dout[tgt] + g)
    dhr = torch.zeros_like(hr).index_add_(0, tgt, g)
    return dict(out=out, dhl=dhl, dhr=dhr,
                datt=(ds.unsqueeze(-1) * lr).sum(0), ds=ds, lr=lr)


def _run(fn, hr, hl, att, tgt, src, n_tgt, slope, dout):
    hr_, hl_, att_ = (v.clone().requires_grad_(True) for v in (hr, hl, att))
    out = fn(hr_, hl_, att_, tgt, src, n_tgt, slope)
    out.backward(dout.to(out.dtype))
    return dict(out=out.detach(), dhl=hl_.grad, dhr=hr_.grad,
                datt=att_.grad)


def _max_err(x, ref):
    return (x.double().cpu() - ref).abs().max().item() if ref.numel() else 0.


def _within_twice(name, fused, comp, ref):
    ef, ec = _max_err(fused, ref), _max_err(comp, ref)
    scale = ref.abs().max().item() if ref.numel() else 0.
    print("%s: fused err %.3e, composition err %.3e, max|ref| %.3e" % (
        name, ef, ec, scale))
    assert ef <= 2 * ec + 1e-6 * scale, name


def _rule3(case, slope=0.2, dtype=torch.float32, keys=KEYS):
    hr, hl, att, tgt, src, n_tgt, dout = case
    hr, hl, dout = (v.to(dtype) for v in (hr, hl, dout))
    ref = _ref64(hr, hl, att, tgt, src, n_tgt, slope, dout)
    fused = _run(gatv2_softmax_aggregate, hr, hl, att, tgt, src, n_tgt,
                 slope, dout)
    comp = _run(gatv2_composition, hr, hl, att, tgt, src, n_tgt, slope,
                dout)
    for k in KEYS:
        assert torch.isfinite(fused[k]).all(), k
        assert fused[k].shape == ref[k].shape, k
    for k in keys:
        _within_twice(k, fused[k], comp[k], ref[k])
    return fused, ref


# --------------------------------------------------------------------------
# CPU: the composition against a per-edge loop
# --------------------------------------------------------------------------
def test_composition_matches_per_edge_loop():
    """Target 2 has no edge, target 1 one edge, target 0 takes source 4
    twice; edges are not sorted."""
    g = torch.Generator().manual_seed(0)
    tgt = torch.tensor([3, 0, 1, 0, 3, 0, 3])
    src = torch.tensor([5, 4, 2, 4, 0, 1, 5])
    n_tgt, n_src, H, C, slope = 4, 7, 2, 3, 0.3
    hr = torch.randn(n_tgt + 1, H, C, generator=g, dtype=torch.float64)
    hl = torch.randn(n_src, H, C, generator=g, dtype=torch.float64)
    att = torch.randn(H, C, generator=g, dtype=torch.float64)
    dout = torch.randn(n_tgt, H, C, generator=g, dtype=torch.float64)
    got = _run(gatv2_softmax_aggregate, hr, hl, att, tgt, src, n_tgt, slope,
               dout)

    E = tgt.numel()
    out = torch.zeros(n_tgt, H, C, dtype=torch.float64)
    dhl, dhr, datt = (torch.zeros_like(v) for v in (hl, hr, att))
    for h in range(H):
        lr = [[max(hl[src[e], h, c] + hr[tgt[e], h, c], 0)
               + slope * min(hl[src[e], h, c] + hr[tgt[e], h, c], 0)
               for c in range(C)] for e in range(E)]
        sc = [sum(att[h, c] * lr[e][c] for c in range(C)) for e in range(E)]
        p = [0.0] * E
        for t in range(n_tgt):
            seg = [e for e in range(E) if tgt[e] == t]
            z = sum(torch.exp(sc[e]) for e in seg)
            for e in seg:
                p[e] = torch.exp(sc[e]) / z
                out[t, h] += p[e] * hl[src[e], h]
        for e in range(E):
            t, s = tgt[e], src[e]
            ds = p[e] * (dout[t, h] @ hl[s, h] - dout[t, h] @ out[t, h])
            for c in range(C):
                u = hl[s, h, c] + hr[t, h, c]
                gec = ds * att[h, c] * (1.0 if u > 0 else slope)
                dhl[s, h, c] += p[e] * dout[t, h, c] + gec
                dhr[t, h, c] += gec
                datt[h, c] += ds * lr[e][c]
    want = dict(out=out, dhl=dhl, dhr=dhr, datt=datt)
    for k in KEYS:
        assert torch.allclose(got[k], want[k], rtol=1e-11, atol=1e-12), k
    assert not got["out"][2].any() and not got["dhr"][2].any()
    assert not got["dhr"][n_tgt:].any()       # hr row past the targets
    assert not got["dhl"][[3, 6]].any()       # sources without an edge
    # and the vectorised reference of the GPU tests is the same thing
    ref = _ref64(hr, hl, att, tgt, src, n_tgt, slope, dout)
    for k in KEYS:
        assert torch.allclose(ref[k], want[k], rtol=1e-11, atol=1e-12), k
    # half precision in, half precision out, fp32 inside
    o16 = gatv2_composition(hr.bfloat16(), hl.bfloat16(), att.float(), tgt,
                            src, n_tgt, slope)
    assert o16.dtype == torch.bfloat16
    assert torch.allclose(o16.double(), out, atol=0.1)


# --------------------------------------------------------------------------
# CPU: layer plumbing
# --------------------------------------------------------------------------
def _layer_graph(seed, n=30, nt=12, E=90, F=8):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.sort(torch.randint(0, nt, (E,), generator=g)).values
    src = torch.randint(0, n - 1, (E,), generator=g)   # node n-1 isolated
    return torch.randn(n, F, generator=g), torch.stack([tgt, src]), nt


def test_layer_state_dict_and_share_weights():
    conv = GATv2Conv(8, 4, heads=3)
    assert not isinstance(conv, GATConv)
    assert conv.use_fused
    assert set(conv.state_dict()) == {"lin_l.weight", "lin_l.bias",
                                      "lin_r.weight", "lin_r.bias", "att",
                                      "bias"}
    assert conv.att.shape == (1, 3, 4) and conv.bias.shape == (12,)
    assert conv.lin_l.weight.shape == (12, 8)
    assert conv.lin_r is not conv.lin_l
    nb = GATv2Conv(8, 4, heads=3, bias=False)
    assert set(nb.state_dict()) == {"lin_l.weight", "lin_r.weight", "att"}
    sh = GATv2Conv(8, 4, heads=3, share_weights=True)
    assert sh.lin_r is sh.lin_l
    assert len(list(sh.parameters())) == 4
    # a state dict loads across the two
    conv.load_state_dict(sh.state_dict())
    assert torch.equal(conv.lin_r.weight, conv.lin_l.weight)
    x, ei, nt = _layer_graph(1)
    assert torch.allclose(conv(x, ei, nt), sh(x, ei, nt), atol=1e-6)


def test_layer_matches_definition_and_concat_false():
    x, ei, nt = _layer_graph(2)
    torch.manual_seed(2)
    for concat in (True, False):
        conv = GATv2Conv(8, 4, heads=3, concat=concat, negative_slope=0.3)
        with torch.no_grad():
            conv.bias.normal_()
            conv.lin_l.bias.normal_()
            conv.lin_r.bias.normal_()
        out = conv(x, ei, nt)
        hl = conv.lin_l(x).view(-1, 3, 4)
        hr = conv.lin_r(x[:nt]).view(-1, 3, 4)
        ref = _ref64(hr, hl, conv.att[0], ei[0], ei[1], nt, 0.3,
                     torch.zeros(nt, 3, 4))["out"]
        ref = (ref.reshape(nt, 12) if concat else ref.mean(1)) \
            + conv.bias.detach().double()
        assert out.shape == (nt, 12 if concat else 4)
        assert torch.allclose(out.double(), ref, atol=1e-5)


def test_layer_tuple_equals_stacked_and_unsorted_equals_sorted():
    x, ei, nt = _layer_graph(3)
    torch.manual_seed(3)
    conv = GATv2Conv(8, 4, heads=2)
    g = torch.Generator().manual_seed(4)
    x_t = torch.randn(nt, 8, generator=g)
    homo = conv(torch.cat([x_t, x]), torch.stack([ei[0], ei[1] + nt]), nt)
    assert torch.allclose(conv((x_t, x), ei), homo, atol=1e-6)
    perm = torch.randperm(ei.size(1), generator=g)
    shuffled = conv(x, ei[:, perm], nt, sorted_by_target=False)
    assert torch.allclose(shuffled, conv(x, ei, nt), atol=1e-6)
    # training with dropout takes the composition and drops something
    drop = GATv2Conv(8, 4, heads=2, dropout=0.5)
    drop.load_state_dict(conv.state_dict())
    drop.train()
    assert not torch.allclose(drop(x, ei, nt), conv(x, ei, nt), atol=1e-6)
    drop.eval()
    assert torch.equal(drop(x, ei, nt), conv(x, ei, nt))


def test_gat_v2_trim_equivalence(ring_graph):
    glt_amd.seed_everything(3)
    ds = Dataset()
    ds.init_graph(edge_index=ring_graph["edge_index"], graph_mode="CPU",
                  num_nodes=ring_graph["num_nodes"])
    ds.init_node_features(ring_graph["feats"], with_gpu=False)
    ds.init_node_labels(ring_graph["labels"])
    loader = NeighborLoader(ds, [2, 2], input_nodes=torch.arange(20),
                            batch_size=10)
    data = next(iter(loader))
    model = GAT(16, 8, 2, out_channels=5, heads=2, v2=True)
    assert all(isinstance(c, GATv2Conv) for c in model.convs)
    assert not any(isinstance(c, GATv2Conv)
                   for c in GAT(16, 8, 2, out_channels=5).convs)
    model.eval()
    x = data.x / ring_graph["num_nodes"]
    with torch.no_grad():
        a = model(x, data.edge_index)[:data.batch_size]
        b = model(x, data.edge_index, data.num_sampled_nodes,
                  data.num_sampled_edges)[:data.batch_size]
    assert a.shape == (data.batch_size, 5)
    assert torch.allclose(a, b, atol=1e-5), (a - b).abs().max()


def _hetero_batch(device, dtype=torch.float32):
    g = torch.Generator().manual_seed(4)
    ets = [("p", "cites", "p"), ("p", "rev_writes", "a"), ("a", "aff", "i")]
    n = {"p": 60, "a": 30, "i": 10}
    x = {t: torch.randn(n[t], 32, generator=g).to(device, dtype) for t in n}
    ei = {}
    for (s_t, r, d_t) in ets:
        E = 4 * n[s_t]
        tgt = torch.sort(torch.randint(0, n[s_t], (E,), generator=g)).values
        src = torch.randint(0, n[d_t], (E,), generator=g)
        ei[(s_t, r, d_t)] = torch.stack([tgt, src]).to(device)
    return ets, x, ei


def test_rgnn_rgatv2_runs_and_skips_multi_gat(monkeypatch):
    def no_multi(*a, **k):
        raise AssertionError("rgatv2 entered the v1 multi-relation path")

    monkeypatch.setattr(HeteroConv, "_multi_gat", no_multi)
    monkeypatch.setattr(HeteroConv, "_batched_gat", no_multi)
    ets, x, ei = _hetero_batch("cpu")
    torch.manual_seed(5)
    model = RGNN(ets, 32, 64, 5, num_layers=2, n_heads=2, model="rgatv2",
                 dropout=0.0)
    convs = [c for layer in model.layers for c in layer.convs.values()]
    assert len(convs) == 6
    assert all(isinstance(c, GATv2Conv) and c.heads == 2
               and c.out_channels == 32 for c in convs)
    out = model(x, ei, predict_type="p")
    assert out.shape == (60, 5) and torch.isfinite(out).all()
    out.pow(2).sum().backward()
    assert all(c.att.grad is not None and c.att.grad.abs().sum() > 0
               for c in model.layers[0].convs.values())


def test_native_fwd_rejects_bad_arguments():
    """Every check fires before a launch (and before the device check, so
    it is seen here, without a GPU)."""
    from glt_amd import _C

    def call(C=4, hdt=torch.float32, adt=torch.float32, idt=torch.long,
             n_off=4, n_tgt=3, H=2):
        return _C.gatv2_fwd(
            torch.zeros(3, H, C, dtype=hdt), torch.zeros(5, H, C, dtype=hdt),
            torch.zeros(H, C, dtype=adt), torch.zeros(6, dtype=idt),
            torch.zeros(n_off, dtype=torch.long), n_tgt, 0.2)

    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        call(hdt=torch.float64)
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        call(hdt=torch.float16)
    with pytest.raises(RuntimeError, match="att must be float32"):
        call(adt=torch.float64)
    with pytest.raises(RuntimeError, match="int64"):
        call(idt=torch.int32)
    with pytest.raises(RuntimeError, match="1 <= C <= 128"):
        call(C=129)
    with pytest.raises(RuntimeError, match="n_tgt \\+ 1"):
        call(n_off=3)
    with pytest.raises(RuntimeError, match="cover all targets"):
        call(n_off=5, n_tgt=4)
    with pytest.raises(RuntimeError, match="one dtype"):
        _C.gatv2_fwd(torch.zeros(3, 2, 4, dtype=torch.bfloat16),
                     torch.zeros(5, 2, 4), torch.zeros(2, 4),
                     torch.zeros(6, dtype=torch.long),
                     torch.zeros(4, dtype=torch.long), 3, 0.2)
    with pytest.raises(RuntimeError, match="contiguous"):
        _C.gatv2_fwd(torch.zeros(3, 2, 8)[:, :, ::2], torch.zeros(5, 2, 4),
                     torch.zeros(2, 4), torch.zeros(6, dtype=torch.long),
                     torch.zeros(4, dtype=torch.long), 3, 0.2)
    with pytest.raises(RuntimeError, match="on the GPU"):
        call()


# --------------------------------------------------------------------------
# GPU: kernels
# --------------------------------------------------------------------------
SEG = [0, 1, 3, 4, 5, 9, 70, 8, 0, 2]   # either side of the 4-edge batch
_cases = {}


def _kernel_case(C, H):
    """n_tgt = 10 < n_src = 40; sources 35.. have no edge; the first two
    edges of the 9-edge segment share their source; the 70-edge hub draws
    from 35 sources, so most repeat.  Built once per (C, H), never
    modified."""
    if (C, H) in _cases:
        return _cases[(C, H)]
    g = torch.Generator().manual_seed(1000 + 10 * C + H)
    n_tgt, n_src = len(SEG), 40
    tgt = torch.repeat_interleave(torch.arange(n_tgt), torch.tensor(SEG))
    src = torch.randint(0, 35, (tgt.numel(),), generator=g)
    first9 = sum(SEG[:5])
    src[first9 + 1] = src[first9]
    case = tuple(v.cuda() if torch.is_tensor(v) else v for v in (
        torch.randn(n_tgt + 2, H, C, generator=g),     # hr: rows to spare
        torch.randn(n_src, H, C, generator=g),
        torch.randn(H, C, generator=g) / C ** 0.5,
        tgt, src, n_tgt, torch.randn(n_tgt, H, C, generator=g)))
    _cases[(C, H)] = case
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("C", [1, 8, 64, 65, 128])
def test_kernels_fp32_within_twice_the_composition(C, H):
    """Check 3.  Also: empty targets, hr rows past the targets and sources
    without edges get exact zeros."""
    case = _kernel_case(C, H)
    fused, _ = _rule3(case)
    assert fused["out"].dtype == torch.float32
    assert not fused["out"][[0, 8]].any()
    assert not fused["dhr"][[0, 8, 10, 11]].any()
    assert not fused["dhl"][35:].any()


@pytest.mark.gpu
def test_kernels_grid_stride():
    """2100 targets x 4 heads = 8400 (target, head) pairs, more than the
    8192 waves of the largest launch."""
    g = torch.Generator().manual_seed(7)
    n_tgt, n_src, H, C = 2100, 2500, 4, 8
    deg = torch.randint(1, 3, (n_tgt,), generator=g)
    tgt = torch.repeat_interleave(torch.arange(n_tgt), deg)
    case = tuple(v.cuda() if torch.is_tensor(v) else v for v in (
        torch.randn(n_tgt, H, C, generator=g),
        torch.randn(n_src, H, C, generator=g),
        torch.randn(H, C, generator=g), tgt,
        torch.randint(0, n_src, (tgt.numel(),), generator=g), n_tgt,
        torch.randn(n_tgt, H, C, generator=g)))
    _rule3(case)


def _scaled_to_100(case):
    hr, hl, att, tgt, src, n_tgt, dout = case
    u = hl.double().cpu()[src.cpu()] + hr.double().cpu()[tgt.cpu()]
    score = (torch.where(u > 0, u, 0.2 * u) * att.double().cpu()).sum(-1)
    att = att * (100.0 / score.abs().max().item())
    return hr, hl, att, tgt, src, n_tgt, dout


@pytest.mark.gpu
@pytest.mark.parametrize("C", [64, 65])
def test_kernels_large_logits(C):
    """Check 4: att scaled until the scores reach +-100; exp of a raw
    score would overflow fp32 at 89.  Everything is finite and inside
    rule 3.

    This case is why the kernels hold the score as a pair of floats.  A
    plain fp32 score near 100 has an ulp of 7.6e-6 and an error of a few
    1e-6, and wherever a segment's two best scores nearly tie that error
    goes into p unreduced and, times att, into every gradient; which of
    two fp32 paths then has the larger maximum over the one or two
    near-tie segments of this graph is a draw (with fp32 scores the
    kernels gave dhl 5.6e-05 against the composition's 1.3e-05 at C = 65
    and missed the rule).  Measured with the pair, fused / composition:
      C = 64: out 2.8e-07 / 8.1e-07, dhl 1.9e-06 / 2.3e-05,
              dhr 2.6e-06 / 1.7e-05, datt 9.0e-07 / 6.4e-06;
      C = 65: out 2.9e-07 / 4.0e-07, dhl 2.7e-06 / 1.3e-05,
              dhr 2.4e-06 / 1.1e-05, datt 8.5e-07 / 3.2e-06."""
    _rule3(_scaled_to_100(_kernel_case(C, 3)))


@pytest.mark.gpu
def test_kernels_large_logits_many_segments():
    """Check 4 on 400 targets x 3 heads, 2-9 edges each: 1200 segments, of
    which roughly a tenth have their two best scores within 2 of each
    other at a score spread of ~33, so each path's maximum is taken over
    about a hundred near-tie draws.  Measured, fused / composition: out
    5.1e-07 / 8.6e-06, dhl 1.1e-05 / 8.4e-05, dhr 7.1e-06 / 7.7e-05, datt
    1.1e-05 / 7.6e-05."""
    g = torch.Generator().manual_seed(12)
    n_tgt, n_src, H, C = 400, 600, 3, 64
    deg = torch.randint(2, 10, (n_tgt,), generator=g)
    tgt = torch.repeat_interleave(torch.arange(n_tgt), deg)
    case = tuple(v.cuda() if torch.is_tensor(v) else v for v in (
        torch.randn(n_tgt, H, C, generator=g),
        torch.randn(n_src, H, C, generator=g),
        torch.randn(H, C, generator=g) / C ** 0.5, tgt,
        torch.randint(0, n_src, (tgt.numel(),), generator=g), n_tgt,
        torch.randn(n_tgt, H, C, generator=g)))
    _rule3(_scaled_to_100(case))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [64, 65])
def test_single_edge_targets_copy_the_source_row(C, dtype):
    """Check 1.  One edge per target: the online softmax starts from p = 1,
    Z = 1 and a zero accumulator, so out = 1 * hl[src] * (1 / 1): the bits
    of hl[src] for any att, in fp32 and (a bf16 value is an fp32 value)
    in bf16."""
    g = torch.Generator().manual_seed(8)
    n_tgt, n_src, H = 50, 70, 3
    hr = (torch.randn(n_tgt, H, C, generator=g) * 30).cuda().to(dtype)
    hl = (torch.randn(n_src, H, C, generator=g) * 30).cuda().to(dtype)
    att = (torch.randn(H, C, generator=g) * 5).cuda()
    tgt = torch.arange(n_tgt).cuda()
    src = torch.randint(0, n_src, (n_tgt,), generator=g).cuda()
    out = gatv2_softmax_aggregate(hr, hl, att, tgt, src, n_tgt)
    assert out.dtype == dtype
    assert torch.equal(out, hl[src])


@pytest.mark.gpu
def test_uniform_softmax_is_exact():
    """Check 2.  att = 0, slope = 0.5, integers in [-2, 2], segment lengths
    1, 2, 4, 8.  Every score is 0, exp(0) = 1, Z = deg, 1 / deg is a power
    of two, so p = 1 / deg exactly and:
      out  = sum(hl) / deg, multiples of 1/8 below 2^5;
      dhl  = sum of dout / deg, the same; the g term is ds * 0 = 0;
      dhr  = sums of ds * 0 * (1 or 0.5) = 0;
      datt = sum_e ds_e * leaky(u_e), ds_e a multiple of 1/64 (p times a
             difference of multiples of 1/8), leaky(u) of 1/2: every term
             and partial sum is a multiple of q = 2^-7, and the test shows
             in fp64 that sum_e |term| / q < 2^24, so the partial sums of
             any order fit fp32's 24 bits.
    expf(0) and 1 / 2^k were not found inexact on gfx950."""
    g = torch.Generator().manual_seed(9)
    deg = torch.tensor([1, 2, 4, 8] * 6)
    n_tgt, n_src, H, C, slope = deg.numel(), 30, 2, 8, 0.5
    tgt = torch.repeat_interleave(torch.arange(n_tgt), deg)
    E = tgt.numel()

    def ints(*shape):
        return torch.randint(-2, 3, shape, generator=g).float()

    hr, hl, dout = ints(n_tgt, H, C), ints(n_src, H, C), ints(n_tgt, H, C)
    att = torch.zeros(H, C)
    src = torch.randint(0, n_src - 3, (E,), generator=g)
    ref = _ref64(hr, hl, att, tgt, src, n_tgt, slope, dout)
    q = 2.0 ** -7
    terms = (ref["ds"].unsqueeze(-1) * ref["lr"]) / q
    assert torch.equal(terms, terms.round())
    assert terms.abs().sum(0).max().item() < 2 ** 24
    assert ref["datt"].abs().max() > 0 and not ref["dhr"].any()
    got = _run(gatv2_softmax_aggregate, hr.cuda(), hl.cuda(), att.cuda(),
               tgt.cuda(), src.cuda(), n_tgt, slope, dout.cuda())
    for k in KEYS:
        assert torch.equal(got[k].double().cpu(), ref[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 65])
def test_kernels_bf16(C):
    """Check 5."""
    hr, hl, att, tgt, src, n_tgt, dout = _kernel_case(C, 3)
    hr, hl, dout = (v.bfloat16() for v in (hr, hl, dout))
    ref = _ref64(hr, hl, att, tgt, src, n_tgt, 0.2, dout)
    f32 = _run(gatv2_softmax_aggregate, hr.float(), hl.float(), att, tgt,
               src, n_tgt, 0.2, dout.float())
    f16 = _run(gatv2_softmax_aggregate, hr, hl, att, tgt, src, n_tgt, 0.2,
               dout)
    for k in ("out", "dhl", "dhr"):
        assert f16[k].dtype == torch.bfloat16
        b32 = _max_err(f32[k], ref[k])
        err = (f16[k].double().cpu() - ref[k]).abs()
        bound = UBF * ref[k].abs() + b32
        print("bf16 %s: max err %.3e, b32 %.3e, max err/bound %.3f" % (
            k, err.max().item(), b32, (err / bound.clamp(min=1e-300)).max()))
        assert (err <= bound).all(), k
    assert f16["datt"].dtype == torch.float32
    comp = _run(gatv2_composition, hr, hl, att, tgt, src, n_tgt, 0.2, dout)
    _within_twice("datt", f16["datt"], comp["datt"], ref["datt"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_backward_is_bit_reproducible(dtype):
    """Check 6, deterministic mode off: no gradient goes through a float
    atomic, every sum has a fixed order."""
    from glt_amd.ops import is_deterministic

    assert not is_deterministic()
    hr, hl, att, tgt, src, n_tgt, dout = _kernel_case(64, 3)
    hr, hl, dout = (v.to(dtype) for v in (hr, hl, dout))
    a = _run(gatv2_softmax_aggregate, hr, hl, att, tgt, src, n_tgt, 0.2, dout)
    b = _run(gatv2_softmax_aggregate, hr, hl, att, tgt, src, n_tgt, 0.2, dout)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_empty_inputs_and_unused_gradients():
    """Check 7, and a source projection that wants no gradient."""
    dev = torch.device("cuda")
    none = torch.zeros(0, dtype=torch.long, device=dev)
    hl = torch.randn(6, 2, 8, device=dev)
    att = torch.randn(2, 8, device=dev)
    for n_tgt in (4, 0):
        hr = torch.randn(n_tgt, 2, 8, device=dev)
        got = _run(gatv2_softmax_aggregate, hr, hl, att, none, none, n_tgt,
                   0.2, torch.ones(n_tgt, 2, 8, device=dev))
        assert got["out"].shape == (n_tgt, 2, 8) and not got["out"].any()
        assert got["dhl"].shape == hl.shape and not got["dhl"].any()
        assert got["dhr"].shape == hr.shape and not got["dhr"].any()
        assert got["datt"].shape == att.shape and not got["datt"].any()
    hr, hl, att, tgt, src, n_tgt, dout = _kernel_case(8, 3)
    ref = _ref64(hr, hl, att, tgt, src, n_tgt, 0.2, dout)
    hr_ = hr.clone().requires_grad_(True)
    gatv2_softmax_aggregate(hr_, hl, att, tgt, src, n_tgt).backward(dout)
    assert torch.allclose(hr_.grad.double().cpu(), ref["dhr"], atol=1e-4)
    with torch.no_grad():
        out = gatv2_softmax_aggregate(hr, hl, att, tgt, src, n_tgt)
    assert torch.allclose(out.double().cpu(), ref["out"], atol=1e-5)


# --------------------------------------------------------------------------
# GPU: layer and models
# --------------------------------------------------------------------------
def _run_module(mod, fwd, x_list, gy):
    mod.zero_grad()
    xs = [v.clone().requires_grad_(True) for v in x_list]
    out = fwd(mod, xs)
    out.backward(gy.to(out.device, out.dtype))
    res = {"out": out.detach()}
    for i, v in enumerate(xs):
        res["dx%d" % i] = v.grad
    seen = set()
    for name, p in mod.named_parameters():
        if id(p) not in seen and p.grad is not None:
            seen.add(id(p))
            res[name] = p.grad.clone()
    return res


def _fused_comp_ref(mod, fwd, x_list, gy, convs_of=lambda m: [m]):
    """Rule 3 on a module: the fp64 copy on the CPU is the reference, the
    module with use_fused = False on the GPU the yardstick."""
    ref = _run_module(copy.deepcopy(mod).double(), fwd,
                      [v.double() for v in x_list], gy.double())
    mod = mod.cuda()
    xs = [v.cuda() for v in x_list]
    fused = _run_module(mod, fwd, xs, gy)
    for c in convs_of(mod):
        c.use_fused = False
    comp = _run_module(mod, fwd, xs, gy)
    for c in convs_of(mod):
        c.use_fused = True
    assert set(fused) == set(ref) == set(comp)
    for k in ref:
        _within_twice(k, fused[k], comp[k], ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["homo", "tuple", "share", "mean"])
def test_gatv2conv_fused_vs_composition_vs_fp64(mode, monkeypatch):
    import glt_amd.ops.gat as gat_ops

    g = torch.Generator().manual_seed(20)
    n, nt, F = 300, 100, 48
    deg = torch.randint(0, 9, (nt,), generator=g)
    tgt = torch.repeat_interleave(torch.arange(nt), deg)
    src = torch.randint(0, n, (tgt.numel(),), generator=g)
    x = torch.randn(n, F, generator=g)
    x_t = torch.randn(nt, F, generator=g)
    torch.manual_seed(21)
    conv = GATv2Conv(F, 24, heads=3, share_weights=mode == "share",
                     concat=mode != "mean")
    gy = torch.randn(nt, 72 if mode != "mean" else 24, generator=g)
    calls = []
    real = gat_ops._GatV2Fused.apply
    monkeypatch.setattr(gat_ops._GatV2Fused, "apply",
                        lambda *a: calls.append(1) or real(*a))

    def fwd(m, xs):
        ei = torch.stack([tgt, src]).to(xs[0].device)
        if mode == "tuple":
            return m((xs[1], xs[0]), ei)
        return m(xs[0], ei, num_target=nt)

    _fused_comp_ref(conv, fwd, [x, x_t] if mode == "tuple" else [x], gy)
    assert len(calls) == 1     # the fused run took the kernels, only it


def _gpu_dataset(n, E, seed):
    g = torch.Generator().manual_seed(seed)
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack([
        torch.randint(0, n, (E,), generator=g),
        torch.randint(0, n, (E,), generator=g)]), graph_mode="CUDA",
        num_nodes=n, device=0)
    ds.init_node_features(torch.randn(n, 32, generator=g), split_ratio=1.0,
                          device=0)
    ds.init_node_labels(torch.randint(0, 5, (n,), generator=g))
    return ds


@pytest.mark.gpu
def test_gat_v2_on_loader_batch_with_trim_lists():
    dev = torch.device("cuda", 0)
    glt_amd.seed_everything(22)
    loader = NeighborLoader(_gpu_dataset(2000, 16000, 22), [5, 5],
                            input_nodes=torch.arange(256), batch_size=128,
                            device=dev, to_device=dev)
    data = next(iter(loader))
    trims = (data.num_sampled_nodes, data.num_sampled_edges)
    bs = data.batch_size
    torch.manual_seed(23)
    model = GAT(32, 16, 2, out_channels=5, heads=2, v2=True)
    ei = data.edge_index.cpu()
    gy = torch.randn(bs, 5)

    def fwd(m, xs):
        return m(xs[0], ei.to(xs[0].device), *trims)[:bs]

    _fused_comp_ref(model, fwd, [data.x.cpu()], gy,
                    convs_of=lambda m: list(m.convs))
    # bf16 features train too
    model.zero_grad()
    out = model(data.x.bfloat16(), data.edge_index, *trims)[:bs]
    loss = torch.nn.functional.cross_entropy(out.float(), data.y[:bs])
    loss.backward()
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())


@pytest.mark.gpu
def test_rgnn_rgatv2_fused_vs_composition():
    ets, x, ei = _hetero_batch("cpu")
    torch.manual_seed(24)
    model = RGNN(ets, 32, 64, 5, num_layers=2, n_heads=2, model="rgatv2",
                 dropout=0.0)
    keys = sorted(x)
    gy = torch.randn(60, 5, generator=torch.Generator().manual_seed(25))

    def fwd(m, xs):
        dev = xs[0].device
        return m(dict(zip(keys, xs)), {k: v.to(dev) for k, v in ei.items()},
                 predict_type="p")

    _fused_comp_ref(
        model, fwd, [x[k] for k in keys], gy,
        convs_of=lambda m: [c for layer in m.layers
                            for c in layer.convs.values()])

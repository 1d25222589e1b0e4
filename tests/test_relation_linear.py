"""ops.relation_linear, the grouped K-segmented projection, and the
RGNN / HeteroConv switch that reaches it.

    Y_g[i, :] = act( sum over segments s of g with i < M_s of
                     ( x_s[i, :] @ W_s^T + b_s ) )

1. Exact arithmetic: x, W, dY integers in [-3, 3], biases in [-8, 8]; every
   partial sum is an integer far below 2^24, so the fp32-accumulating
   kernels must return the int64 evaluation of the definition, rounded
   once to bf16 where the output is bf16, bit for bit.
2. Derived bound on randn inputs, as part B of test_gemm_family.py: with
   u = 2^-24 and gamma_n = n u / (1 - n u), any order of the group's fp32
   sum of K_tot products and S biases errs by at most
   gamma_{K_tot + S + 5} * (sum_s |x_s| @ |W_s|^T + sum_s |b_s|); a bf16
   output adds half a bf16 ulp of |ref| + that.  dW and db: gamma_{M_s+5}.
3. Routing and the torch composition (no GPU).
4. RGNN(fuse_projections=True) equals the per-relation model.
"""
import pytest
import torch

from glt_amd import _C
from glt_amd.ops import relation_linear, relation_linear_uses_kernel

BF16 = torch.bfloat16
U = 2.0 ** -24

# name: (rows per group, [(group, M_s, K_s, N, has bias)], lowest input)
CASES = {
    "one": ([1], [(0, 1, 8, 1, True)], -3),
    "two_groups": ([65, 130], [(0, 65, 8, 72, True), (0, 37, 72, 72, False),
                               (0, 65, 200, 72, True),
                               (1, 130, 72, 257, False),
                               (1, 100, 8, 257, True)], -3),
    "empty": ([0, 70, 5], [(0, 0, 8, 40, True), (1, 0, 16, 24, True),
                           (1, 70, 16, 24, False), (2, 5, 8, 16, False)], -3),
    "nonneg": ([65], [(0, 65, 200, 136, True), (0, 37, 72, 136, False)], 0),
}


def _gamma(n):
    return n * U / (1.0 - n * U)


def _half_ulp_bf16(x):
    _, e = torch.frexp(x)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9),
                       torch.zeros_like(x))


def _reference(xs, ws, bs, dys, group, rows, relu):
    """The definition and its gradients in the dtype of the inputs (int64
    or fp64), plus the magnitudes the bounds of part 2 are built from."""
    G = len(rows)
    n_of = {g: w.size(0) for g, w in zip(group, ws)}
    pre = [torch.zeros(rows[g], n_of.get(g, 0), dtype=xs[0].dtype)
           for g in range(G)]
    mag = [p.clone() for p in pre]
    for x, w, b, g in zip(xs, ws, bs, group):
        m = x.size(0)
        pre[g][:m] += x @ w.t() + (0 if b is None else b)
        mag[g][:m] += x.abs() @ w.abs().t() + (0 if b is None else b.abs())
    ys = [p.clamp(min=0) if relu else p for p in pre]
    dym = [dy * (p > 0) if relu else dy for dy, p in zip(dys, pre)]
    out = {"y": ys, "ymag": mag, "dx": [], "dxmag": [], "dw": [], "dwmag": [],
           "db": [], "dbmag": []}
    for x, w, g in zip(xs, ws, group):
        d = dym[g][:x.size(0)]
        out["dx"].append(d @ w)
        out["dxmag"].append(d.abs() @ w.abs())
        out["dw"].append(d.t() @ x)
        out["dwmag"].append(d.abs().t() @ x.abs())
        out["db"].append(d.sum(0))
        out["dbmag"].append(d.abs().sum(0))
    return out


def _make(name, integer, seed=0):
    rows, segs, lo = CASES[name]
    g = torch.Generator().manual_seed(seed)
    group = [s[0] for s in segs]
    if integer:
        def draw(shape, lo=lo, hi=3):
            return torch.randint(lo, hi + 1, shape, generator=g)
    else:
        def draw(shape, lo=0, hi=0):
            return torch.randn(shape, generator=g).to(BF16).double()
    xs = [draw((m, k)) for _, m, k, _, _ in segs]
    ws = [draw((n, k)) for _, _, k, n, _ in segs]
    if integer:
        bs = [draw((n,), -8 if lo else 0, 8) if hb else None
              for _, _, _, n, hb in segs]
    else:   # biases stay fp32 in the op
        bs = [torch.randn(n, generator=g).double() if hb else None
              for _, _, _, n, hb in segs]
    n_of = {s[0]: s[3] for s in segs}
    dys = [draw((rows[i], n_of.get(i, 0)), -3) for i in range(len(rows))]
    return xs, ws, bs, dys, group, rows


def _run_gpu(xs, ws, bs, dys, group, rows, relu):
    xd = [x.to(BF16).cuda().requires_grad_(True) for x in xs]
    wd = [w.float().cuda().requires_grad_(True) for w in ws]
    bd = [None if b is None else b.float().cuda().requires_grad_(True)
          for b in bs]
    assert relation_linear_uses_kernel(xd, wd, group, rows)
    ys = relation_linear(xd, wd, bd, group, rows, relu=relu)
    torch.autograd.backward(ys, [dy.to(BF16).cuda() for dy in dys])
    torch.cuda.synchronize()
    return ys, xd, wd, bd


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_relation_linear_exact(name, relu):
    xs, ws, bs, dys, group, rows = _make(name, integer=True)
    ref = _reference(xs, ws, bs, dys, group, rows, relu)
    if name == "nonneg":    # the single rounding is exercised
        v = ref["y"][0]
        assert (v.float().to(BF16).double() != v.double()).sum() > 50
    ys, xd, wd, bd = _run_gpu(xs, ws, bs, dys, group, rows, relu)
    for g, y in enumerate(ys):
        assert y.dtype == BF16
        assert torch.equal(y.cpu(), ref["y"][g].float().to(BF16)), ("Y", g)
    for s in range(len(xs)):
        assert torch.equal(xd[s].grad.cpu(),
                           ref["dx"][s].float().to(BF16)), ("dX", s)
        assert torch.equal(wd[s].grad.cpu(), ref["dw"][s].float()), ("dW", s)
        if bd[s] is not None:
            assert torch.equal(bd[s].grad.cpu(),
                               ref["db"][s].float()), ("db", s)


def _assert_bounded(got, ref, e32, bf16_out, what):
    bound = _half_ulp_bf16(ref.abs() + e32) + e32 if bf16_out else e32
    err = (got.detach().cpu().double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                    torch.where(err > 0, torch.full_like(err, float("inf")),
                                torch.zeros_like(err)))
    r = r.max().item() if r.numel() else 0.0
    print("RELATION_BOUND %s: max err/bound %.3g" % (what, r))
    assert r <= 1.0, "%s: max err/bound %.3g" % (what, r)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
def test_relation_linear_bound(relu):
    """ReLU is 1-Lipschitz, so the forward bound holds after it.  With relu
    the backward is checked against the kernel's own mask (a pre-activation
    within the bound of 0 may round to either side): Y_kernel > 0."""
    name = "two_groups"
    xs, ws, bs, dys, group, rows = _make(name, integer=False, seed=1)
    _, segs, _ = CASES[name]
    ys, xd, wd, bd = _run_gpu(xs, ws, bs, dys, group, rows, relu)
    ref = _reference(xs, ws, bs, dys, group, rows, relu)
    for g, y in enumerate(ys):
        mine = [s for s in segs if s[0] == g]
        n = sum(s[2] for s in mine) + len(mine) + 5
        _assert_bounded(y, ref["y"][g], _gamma(n) * ref["ymag"][g], True,
                        "Y[%d] relu=%s" % (g, relu))
    if relu:
        dys = [dy * (y.detach().cpu() > 0) for dy, y in zip(dys, ys)]
        ref = _reference(xs, ws, bs, dys, group, rows, False)
    for s, (_, m, k, n, hb) in enumerate(segs):
        _assert_bounded(xd[s].grad, ref["dx"][s],
                        _gamma(n + 5) * ref["dxmag"][s], True, "dX[%d]" % s)
        _assert_bounded(wd[s].grad, ref["dw"][s],
                        _gamma(m + 5) * ref["dwmag"][s], False, "dW[%d]" % s)
        if hb:
            _assert_bounded(bd[s].grad, ref["db"][s],
                            _gamma(m + 5) * ref["dbmag"][s], False,
                            "db[%d]" % s)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wide", "narrow"])
@pytest.mark.parametrize("shape", [(65, 72, 136), (130, 200, 257)],
                         ids=lambda s: "x".join(map(str, s)))
def test_relation_linear_one_segment_is_gemm_bt(shape, which, monkeypatch):
    """One group of one segment is the dense projection: relation_gemm_kernel
    and gemm_bt_wide_kernel run one K loop and one epilogue, and
    test_gemm_bt_wide.py pins the 64x64 kernel to the wide one, so all
    three agree bit for bit on real-valued input.  The shapes give a partial
    row tile and a K tail inside a 64-step; N = 136 a dead wave and 16-byte
    rows, N = 257 element stores and a one-column tile."""
    M, K, N = shape
    monkeypatch.delenv("GLT_GEMM_PERSIST", raising=False)
    monkeypatch.setenv("GLT_GEMM_BT", which)
    assert _C.gemm_bt_bf16_plan(M, K, N)[0] == which
    g = torch.Generator().manual_seed(70 + M)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    w = torch.randn(N, K, generator=g).to(BF16).cuda()
    b = torch.randn(N, generator=g).cuda()
    assert relation_linear_uses_kernel([x], [w], [0], [M])
    for bias in (b, None):
        for relu in (False, True):
            y, = relation_linear([x], [w], [bias], [0], [M], relu=relu)
            want = _C.gemm_bt_bf16(x, w, bias, relu, False)
            assert y.dtype == want.dtype == BF16
            assert torch.equal(y, want), (bias is not None, relu)


def test_relation_linear_composition_and_validation():
    xs, ws, bs, dys, group, rows = _make("two_groups", integer=False, seed=2)
    ref = _reference(xs, ws, bs, dys, group, rows, True)
    f = [t.float() for t in xs]
    assert not relation_linear_uses_kernel(f, ws, group, rows)   # CPU
    ys = relation_linear(f, [w.float() for w in ws],
                         [None if b is None else b.float() for b in bs],
                         group, rows, relu=True)
    for y, want in zip(ys, ref["y"]):
        assert y.dtype == torch.float32
        assert torch.allclose(y.double(), want, rtol=1e-4, atol=1e-4)
    assert [tuple(y.shape) for y in relation_linear([], [], [], [], [3])] \
        == [(3, 0)]
    x, w = torch.zeros(4, 8), torch.zeros(5, 8)
    for bad in [dict(rows=[3]), dict(ws=[w, torch.zeros(6, 8)]),
                dict(xs=[x, x.to(BF16)]), dict(ws=[w, w.double()])]:
        with pytest.raises(ValueError):
            relation_linear(bad.get("xs", [x, x]), bad.get("ws", [w, w]),
                            [None, None], [0, 0], bad.get("rows", [4]))


@pytest.mark.gpu
def test_relation_linear_routing():
    x = torch.zeros(16, 24, dtype=BF16, device="cuda")
    w = torch.zeros(8, 16, device="cuda")

    def uses(t, wt=w):
        return relation_linear_uses_kernel([t], [wt], [0], [t.size(0)])
    assert uses(x[:, :16])                        # row-strided, aligned
    assert not uses(x[:, :9], w[:, :9])           # odd K
    assert not uses(x[:, 4:20])                   # misaligned view
    assert not uses(x[:, :16].float())            # fp32
    assert not uses(x[:, :16].cpu(), w.cpu())     # CPU


def _plumbing(device, dtype):
    from glt_amd.models import RGNN

    g = torch.Generator().manual_seed(5)
    etypes = [("a", "to", "b"), ("a", "self", "a")]
    # edge_index[0] indexes the first type of the key, sorted, in-degree
    # <= 4; the targets of a->b cover only a prefix of a's 70 rows
    ei = {etypes[0]: torch.stack([torch.arange(40).repeat_interleave(3),
                                  torch.randint(0, 33, (120,), generator=g)]),
          etypes[1]: torch.stack([torch.arange(70).repeat_interleave(4),
                                  torch.randint(0, 70, (280,), generator=g)])}
    x = {"a": torch.randint(-1, 2, (70, 8), generator=g),
         "b": torch.randint(-1, 2, (33, 8), generator=g)}
    ei = {k: v.to(device) for k, v in ei.items()}
    x = {k: v.to(device=device, dtype=dtype) for k, v in x.items()}
    models = [RGNN(etypes, 8, 32, 3, num_layers=1, model="rsage",
                   sage_aggr="sum", fuse_projections=f).to(device).eval()
              for f in (False, True)]
    state = {k: torch.randint(-1, 2, v.shape, generator=g).float()
             for k, v in models[0].state_dict().items()}
    outs = []
    for m in models:
        m.load_state_dict(state)
        logits = m(x, ei)
        sum(v.float().sum() for v in logits.values()).backward()
        outs.append((logits, {k: p.grad for k, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = outs
    assert l0.keys() == l1.keys() and g0.keys() == g1.keys()
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert any(v.abs().sum() > 0 for v in l0.values())


def test_rgnn_fuse_projections_cpu():
    _plumbing("cpu", torch.float32)


@pytest.mark.gpu
def test_rgnn_fuse_projections_bf16():
    _plumbing("cuda", BF16)

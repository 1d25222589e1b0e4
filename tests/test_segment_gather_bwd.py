"""Atomic-free segment-mean backward: the source-side index
(_C.segment_transpose), the gather kernels (_C.segment_mean[_cat]_bwd_gather)
and their routing through segment_mean[_cat], cast_linear, SAGEConv and
GraphSAGE.

In deterministic mode every term is snapped to a grid on which fp32 sums
below 2^6 max|dy| are exact, so the gather path (sum per source row, in
list order) and the atomic path (sum in arrival order) must agree bit
for bit; the tests assert on their own inputs that every sum stays inside
that headroom.  Plain mode is checked against an fp64 reference with the
bound test_segment_mean.py uses, and for run-to-run identity.
"""
import pytest
import torch

from glt_amd import _C

gpu = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
H = 6  # kGridHeadroomBits


# --------------------------------------------------------------------------
# index
# --------------------------------------------------------------------------
def _ref_transpose(col, n_src):
    _, idx = torch.sort(col, stable=True)
    off = torch.zeros(n_src + 1, dtype=torch.long, device=col.device)
    if col.numel():
        off[1:] = torch.bincount(col, minlength=n_src).cumsum(0)
    return off, idx


def _index_case(name):
    g = torch.Generator(device="cuda").manual_seed(11)

    def rnd(lo, hi, n):
        return torch.randint(lo, hi, (n,), device="cuda", generator=g)

    if name == "no_edges":
        return rnd(0, 1, 0), 7
    if name == "one_source_holds_all":
        return torch.full((1000,), 17, device="cuda"), 50
    if name == "empty_both_ends":
        return rnd(100, 900, 3000), 1000
    if name == "bit_range_k8":      # n_src = 2^8 + 1, edges at col = 2^8
        col = rnd(0, 257, 2000)
        col[::97] = 256
        return col, 257
    if name == "bit_range_k18":
        col = rnd(0, 2 ** 18 + 1, 5000)
        col[::97] = 2 ** 18
        return col, 2 ** 18 + 1
    if name == "grid_stride_edges":
        # more edges and sources than the boundary kernel has threads
        # (2048 blocks x 256)
        return rnd(0, 540_000, 530_000), 540_000
    if name == "grid_stride_head_tail":
        # head [0, key[0]] and tail (key[E-1], n_src] both longer than
        # the grid
        return rnd(600_000, 650_000, 2000), 1_300_000
    raise AssertionError(name)


@gpu
@pytest.mark.parametrize("name", [
    "no_edges", "one_source_holds_all", "empty_both_ends", "bit_range_k8",
    "bit_range_k18", "grid_stride_edges", "grid_stride_head_tail"])
def test_transpose_is_stable_sort_plus_offsets(name):
    col, n_src = _index_case(name)
    ref_off, ref_idx = _ref_transpose(col, n_src)
    off, pos = _C.segment_transpose(col, n_src)
    assert off.dtype == torch.long and off.shape == (n_src + 1,)
    assert pos.dtype == torch.long and pos.shape == col.shape
    assert torch.equal(off, ref_off)
    assert torch.equal(pos, ref_idx)        # ascending e within a list
    # with tgt the lists carry tgt[e], in the same order
    tgt = torch.sort(torch.randint(0, 5000, col.shape, device="cuda"))[0]
    off_t, in_tgt = _C.segment_transpose(col, n_src, tgt)
    assert torch.equal(off_t, ref_off)
    assert torch.equal(in_tgt, tgt[ref_idx])


@gpu
def test_transpose_rejects_bad_arguments():
    col = torch.zeros(5, dtype=torch.long, device="cuda")
    bad = [(col.int(), 6, None), (col.cpu(), 6, None),
           (col.repeat(2)[::2], 6, None), (col.view(1, 5), 6, None),
           (col, -1, None), (col, 0, None),
           (col, 6, col[:4]), (col, 6, col.int()), (col, 6, col.cpu())]
    for c, n, t in bad:
        with pytest.raises(RuntimeError, match="segment"):
            _C.segment_transpose(c, n, t)


# --------------------------------------------------------------------------
# kernels
# --------------------------------------------------------------------------
def _graph(degs, n_src, seed, duplicates=True):
    """Edges sorted by target with degs[t] edges each; with duplicates the
    second edge of every target repeats its first (t, c) pair."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_tgt = degs.numel()
    tgt = torch.arange(n_tgt, device="cuda").repeat_interleave(degs)
    off = torch.zeros(n_tgt + 1, dtype=torch.long, device="cuda")
    off[1:] = degs.cumsum(0)
    col = torch.randint(0, n_src, (tgt.numel(),), device="cuda", generator=g)
    if duplicates:
        two = (degs >= 2).nonzero().flatten()
        col[off[two] + 1] = col[off[two]]
    return tgt, col, off


def _wide_dy(rows, cols, dtype, seed):
    """Values spread over six decades, like real activation gradients."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (-6.0 * torch.rand(rows, cols, device="cuda", generator=g))
    return (torch.randn(rows, cols, device="cuda", generator=g) * mag).to(
        dtype)


def _atomic(dy, col, off, n_src, det, cat):
    fn = _C.segment_mean_cat_bwd if cat else _C.segment_mean_bwd
    return fn(dy, col, off, n_src, det)


def _gather(dy, tgt, col, off, n_src, det, cat, mask=None):
    src_off, in_tgt = _C.segment_transpose(col, n_src, tgt)
    fn = _C.segment_mean_cat_bwd_gather if cat else _C.segment_mean_bwd_gather
    return fn(dy, col, off, n_src, det, src_off, in_tgt, mask)


def _degs(n_tgt, deg):
    """deg edges per target, every 7th target none."""
    d = torch.full((n_tgt,), deg, device="cuda")
    d[::7] = 0
    return d


def _assert_bits_equal_atomic(n_tgt, n_src, degs, F, dtype, cat, seed):
    tgt, col, off = _graph(degs, n_src, seed)
    # every dx element sums at most max in-degree + 1 (root) terms of at
    # most max|dy| each: below 2^H max|dy|, where snapped sums are exact
    assert torch.bincount(col, minlength=n_src).max().item() + 1 < 2 ** H
    dy = _wide_dy(n_tgt, 2 * F if cat else F, dtype, seed + 1)
    ref = _atomic(dy, col, off, n_src, True, cat).to(dtype)
    got = _gather(dy, tgt, col, off, n_src, True, cat)
    assert got.dtype == dtype and got.shape == (n_src, F)
    assert torch.equal(got, ref)
    assert ref.abs().sum().item() > 0


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
@pytest.mark.parametrize("F", [2, 33, 130, 256])
def test_deterministic_bits_equal_atomic_path(dtype, cat, F):
    _assert_bits_equal_atomic(4000, 4100, _degs(4000, 10), F, dtype, cat, 0)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_deterministic_bits_equal_every_row_a_target(dtype, cat):
    _assert_bits_equal_atomic(4000, 4000, _degs(4000, 10), 130, dtype, cat, 2)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_deterministic_bits_equal_grid_stride(dtype, cat):
    """More source rows than the 8192 waves of the largest grid (four
    times as many): most are reached only by the stride loop, through the
    prefetched next block."""
    n_tgt, n_src = 33_000, 8300 * 4
    g = torch.Generator(device="cuda").manual_seed(5)
    degs = torch.randint(0, 3, (n_tgt,), device="cuda", generator=g)
    _assert_bits_equal_atomic(n_tgt, n_src, degs, 4, dtype, cat, 6)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_rows_without_contribution_are_exact_zeros(dtype, cat):
    n_tgt, n_src, F = 64, 6000, 130
    tgt, col, off = _graph(torch.full((n_tgt,), 3, device="cuda"), n_src, 7)
    dy = _wide_dy(n_tgt, 2 * F if cat else F, dtype, 8)
    src_off, in_tgt = _C.segment_transpose(col, n_src, tgt)
    fn = _C.segment_mean_cat_bwd_gather if cat else _C.segment_mean_bwd_gather
    # the output block is what the allocator just got back, full of NaNs
    junk = torch.full((n_src, F), float("nan"), device="cuda", dtype=dtype)
    del junk
    dx = fn(dy, col, off, n_src, True, src_off, in_tgt)
    lonely = torch.ones(n_src, dtype=torch.bool, device="cuda")
    lonely[col] = False
    if cat:
        lonely[:n_tgt] = False
    else:
        assert lonely[:n_tgt].any()     # targets without in-edges count too
    assert lonely[n_tgt:].sum().item() > 5000
    bits = dx[lonely].view(torch.int16 if dtype == BF16 else torch.int32)
    assert not bits.any()               # +0, not -0, not NaN
    assert torch.isfinite(dx.float()).all()


def _ref64(dy, tgt, col, off, n_src, cat):
    """fp64 reference, sum of |terms| and number of terms per dx row."""
    d = dy.double()
    n_tgt = d.size(0)
    F = d.size(1) // 2 if cat else d.size(1)
    deg = (off[1:] - off[:-1]).double().clamp(min=1)
    terms = d[tgt, :F] / deg[tgt].unsqueeze(1)
    ref = torch.zeros(n_src, F, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    ref.index_add_(0, col, terms)
    mag.index_add_(0, col, terms.abs())
    cnt = torch.bincount(col, minlength=n_src).double()
    if cat:
        ref[:n_tgt] += d[:, F:]
        mag[:n_tgt] += d[:, F:].abs()
        cnt[:n_tgt] += 1
    return ref, mag, cnt


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_plain_mode_within_fp32_bound_and_reproducible(dtype, cat):
    n_tgt, n_src, F = 4000, 4100, 130
    tgt, col, off = _graph(_degs(n_tgt, 10), n_src, 9)
    dy = _wide_dy(n_tgt, 2 * F if cat else F, dtype, 10)
    runs = [_gather(dy, tgt, col, off, n_src, False, cat) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    ref, mag, cnt = _ref64(dy, tgt, col, off, n_src, cat)
    bound = (cnt.unsqueeze(1) + 2) * 2.0 ** -24 * mag
    if dtype == BF16:   # one rounding of the sum to bf16
        bound = 2.0 ** -8 * (ref.abs() + bound) + bound
    err = (runs[0].double() - ref).abs()
    print("max err/bound %.3f" % (
        err / bound.clamp(min=1e-300)).max().item())
    assert (err <= bound).all()


@gpu
def test_plain_mode_hub_within_sequential_sum_bound():
    """4096 edges into source row 0, summed by one wave in list order:
    within the sequential fp32 bound (n - 1) * 2^-24 * sum|terms|."""
    n_tgt, n_src, F = 4096, 4096, 64
    tgt = torch.arange(n_tgt, device="cuda")
    col = torch.zeros(n_tgt, dtype=torch.long, device="cuda")
    off = torch.arange(n_tgt + 1, device="cuda")
    dy = 1.0 + 0.5 * torch.rand(n_tgt, F, device="cuda")
    dx = _gather(dy, tgt, col, off, n_src, False, False)
    ref = dy.double().sum(0)
    bound = (n_tgt - 1) * 2.0 ** -24 * dy.double().abs().sum(0)
    err = (dx[0].double() - ref).abs()
    print("max err %.3e, min bound %.3e" % (err.max().item(),
                                            bound.min().item()))
    assert (err <= bound).all()
    assert not dx[1:].any()
    # deterministic mode, past the headroom: same bound plus the snaps
    dxd = _gather(dy, tgt, col, off, n_src, True, False)
    amax = dy.abs().max().item()
    import math
    q = 2.0 ** (math.frexp(amax)[1] + H - 24)
    assert ((dxd[0].double() - ref).abs() <= bound + n_tgt * q / 2).all()


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
@pytest.mark.parametrize("F", [33, 256])
def test_mask_is_threshold_backward(dtype, cat, F):
    n_tgt, n_src = 500, 640
    tgt, col, off = _graph(_degs(n_tgt, 4), n_src, 12)
    dy = _wide_dy(n_tgt, 2 * F if cat else F, dtype, 13)
    g = torch.Generator(device="cuda").manual_seed(14)
    # zeros (+0 and -0), positives, negatives and a NaN; rows past n_src
    # are allowed and ignored
    mask = torch.randn(n_src + 3, F, device="cuda", generator=g)
    mask[torch.rand(n_src + 3, F, device="cuda", generator=g) < 0.2] = 0.0
    mask[1, 0] = -0.0
    mask[2, 1] = float("nan")
    mask = mask.to(dtype)
    plain = _gather(dy, tgt, col, off, n_src, True, cat)
    got = _gather(dy, tgt, col, off, n_src, True, cat, mask)
    ref = torch.ops.aten.threshold_backward(plain, mask[:n_src], 0)
    ib = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(got.view(ib), ref.view(ib))
    masked = mask[:n_src] <= 0
    assert masked.any() and not got.view(ib)[masked].any()      # +0
    assert torch.equal(got[2, 1], plain[2, 1])                  # NaN passes


@gpu
def test_gather_rejects_bad_arguments_and_handles_empty_shapes():
    n_tgt, n_src, F = 4, 6, 8
    tgt, col, off = _graph(torch.full((n_tgt,), 2, device="cuda"), n_src, 15)
    dy = torch.randn(n_tgt, F, device="cuda")
    src_off, in_tgt = _C.segment_transpose(col, n_src, tgt)
    ok = dict(dy=dy, col=col, offsets=off, n_src=n_src,
              order_independent=True, src_off=src_off, in_edge=in_tgt)
    _C.segment_mean_bwd_gather(**ok)
    bad = [dict(src_off=src_off[:-1]), dict(src_off=src_off.int()),
           dict(src_off=src_off.cpu()), dict(in_edge=in_tgt[:-1]),
           dict(in_edge=in_tgt.int()), dict(in_edge=in_tgt.cpu()),
           dict(col=col.int()), dict(offsets=off[:-1]), dict(dy=dy.double()),
           dict(dy=dy.cpu()), dict(mask=dy.new_zeros(n_src - 1, F)),
           dict(mask=dy.new_zeros(n_src, F + 1)),
           dict(mask=dy.new_zeros(n_src, F).to(BF16)),
           dict(mask=dy.new_zeros(n_src, 2 * F)[:, ::2]),
           dict(mask=dy.new_zeros(n_src, F).cpu())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="segment"):
            _C.segment_mean_bwd_gather(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="even"):
        _C.segment_mean_cat_bwd_gather(**{**ok, "dy": dy[:, :3]})
    with pytest.raises(RuntimeError, match="prefix"):
        _C.segment_mean_cat_bwd_gather(**{**ok, "n_src": 2,
                                          "src_off": src_off[:3]})
    # no channels / no targets: zeros of dy's dtype, no launch
    z = _C.segment_mean_bwd_gather(**{**ok, "dy": dy[:, :0]})
    assert z.shape == (n_src, 0)
    e_off, e_in = _C.segment_transpose(col[:0], n_src, tgt[:0])
    for fn, w in ((_C.segment_mean_bwd_gather, F),
                  (_C.segment_mean_cat_bwd_gather, 2 * F)):
        z = fn(dy.new_zeros(0, w).to(BF16), col[:0], off[:1], n_src, True,
               e_off, e_in)
        assert z.shape == (n_src, F) and z.dtype == BF16 and not z.any()


# --------------------------------------------------------------------------
# routing
# --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_autograd_env_switch_and_relu_input(monkeypatch, cat):
    """GLT_SEGMENT_BWD is read per call; both settings give the same
    bits in deterministic mode, with and without the fused input mask."""
    from glt_amd.ops import (segment_mean, segment_mean_cat,
                             set_deterministic)

    n_tgt, n_src, F = 2000, 2100, 64
    tgt, col, _ = _graph(_degs(n_tgt, 10), n_src, 16)
    x = torch.relu(torch.randn(n_src, F, device="cuda")).to(BF16)
    gy = _wide_dy(n_tgt, 2 * F if cat else F, BF16, 17)
    fn = segment_mean_cat if cat else segment_mean

    def grad(relu_input):
        xx = x.clone().requires_grad_(True)
        fn(xx, tgt, col, n_tgt, relu_input=relu_input).backward(gy)
        return xx.grad

    set_deterministic(True)
    try:
        monkeypatch.delenv("GLT_SEGMENT_BWD", raising=False)
        new, new_m = grad(False), grad(True)
        monkeypatch.setenv("GLT_SEGMENT_BWD", "atomic")
        old, old_m = grad(False), grad(True)
    finally:
        set_deterministic(False)
    assert torch.equal(new, old) and torch.equal(new_m, old_m)
    assert torch.equal(new_m,
                       torch.ops.aten.threshold_backward(new, x, 0))
    assert not torch.equal(new_m, new)


def _loader_batch(dtype):
    import glt_amd
    from glt_amd import Dataset, NeighborLoader

    glt_amd.seed_everything(0)
    n = 20_000
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, n, (200_000,), generator=g)
    dst = torch.randint(0, n, (200_000,), generator=g)
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack([src, dst]), graph_mode="CUDA",
                  num_nodes=n, device=0)
    ds.init_node_features(torch.randn(n, 100, generator=g).to(dtype),
                          split_ratio=1.0, device=0)
    ds.init_node_labels(torch.randint(0, 47, (n,), generator=g))
    dev = torch.device("cuda", 0)
    loader = NeighborLoader(ds, [5, 5, 5], input_nodes=torch.arange(300),
                            batch_size=300, device=dev, to_device=dev)
    data = next(iter(loader))
    loader.shutdown()
    return data


@pytest.fixture(scope="module")
def batches():
    return {dt: _loader_batch(dt) for dt in (F32, BF16)}


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
def test_graphsage_grads_equal_atomic_path(monkeypatch, batches, dtype,
                                           dropout):
    from glt_amd.models import GraphSAGE
    from glt_amd.ops import set_deterministic

    data = batches[dtype]
    assert data.x.dtype == dtype
    torch.manual_seed(3)
    model = GraphSAGE(100, 256, 3, 47, dropout=dropout).to("cuda").train()

    def step():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(4)    # same dropout masks in both runs
        out = model(data.x, data.edge_index, data.num_sampled_nodes,
                    data.num_sampled_edges)[:data.batch_size]
        loss = torch.nn.functional.cross_entropy(
            out.float(), data.y[:data.batch_size])
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in model.parameters()]

    x0 = data.x[:sum(int(v) for v in data.num_sampled_nodes[:3])]
    set_deterministic(True)
    try:
        monkeypatch.delenv("GLT_SEGMENT_BWD", raising=False)
        fused = model._relu_mask_by_consumer(x0, model.convs[0],
                                             model.convs[1])
        loss_new, grads_new = step()
        monkeypatch.setenv("GLT_SEGMENT_BWD", "atomic")
        assert not model._relu_mask_by_consumer(x0, model.convs[0],
                                                model.convs[1])
        loss_old, grads_old = step()
    finally:
        set_deterministic(False)
    # the mask moves only for bf16 batches (cast_linear) without dropout
    assert fused == (dtype == BF16 and dropout == 0.0)
    assert torch.equal(loss_new, loss_old)
    assert len(grads_new) == 6
    for a, b in zip(grads_new, grads_old):
        assert a.abs().sum().item() > 0
        assert torch.equal(a, b)


def test_mask_flags_raise_where_they_cannot_be_honoured():
    """CPU tensors take neither the fused aggregation nor cast_linear: a
    conv told to apply (or to leave) the mask raises instead of dropping
    it."""
    from glt_amd.models import GraphSAGE
    from glt_amd.models.layers import SAGEConv
    from glt_amd.ops import cast_linear

    conv = SAGEConv(8, 8)
    x = torch.randn(10, 8)
    ei = torch.tensor([[0, 0, 1], [3, 4, 5]])
    assert conv(x, ei, 2).shape == (2, 8)
    with pytest.raises(ValueError, match="relu_input"):
        conv(x, ei, 2, relu_input=True)
    with pytest.raises(ValueError, match="relu_grad_by_consumer"):
        conv(x, ei, 2, fuse_relu=True, relu_grad_by_consumer=True)
    with pytest.raises(ValueError, match="relu_grad_by_consumer"):
        cast_linear(x.repeat(1, 2).to(BF16), conv.lin.weight, conv.lin.bias,
                    relu=False,
                    relu_grad_by_consumer=True)
    model = GraphSAGE(8, 8, 2)
    assert not model._relu_mask_by_consumer(x, model.convs[0],
                                            model.convs[1])
    assert not model._relu_mask_by_consumer(x.to(BF16), model.convs[0],
                                            model.convs[1])
    out = model(x, ei)      # the CPU path is unchanged
    assert out.shape == (10, 8)

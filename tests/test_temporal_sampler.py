"""Temporal neighbour sampling: _C.sample_neighbors_temporal (CPU twin and
HIP kernels), Topology(edge_times=), NeighborSampler / NeighborLoader with
time_attr=.

The contract (docs/kernels.md, "Temporal sampling"): edge position q of row
s[i] is valid iff time(q) <= t[i]; count = min(k, p) (p for k < 0);
'uniform' emits the valid edges in row order when p <= k and k distinct
valid edges otherwise; 'last' emits the count greatest edges under
"(time, row position) ascending", greatest first.  The reference everywhere
is a brute-force Python loop over the CSR on the CPU.

The uniformity bound is the binomial 6-sigma bound, derived, not fitted:
each of the p = 100 valid edges is drawn with probability q = k / p = 0.1
per slot, so over n = 20000 slots its hit count c has mean n*q = 2000 and
standard deviation sqrt(n*q*(1-q)) = 42.4; |c - 2000| <= 6 * 42.4 = 255.
Over 100 edges the false-alarm probability is below 1e-6.
"""
import math

import pytest
import torch

import glt_amd
from glt_amd import _C, Dataset, NeighborLoader
from glt_amd.data import Graph, Topology
from glt_amd.sampler import (EdgeSamplerInput, NeighborSampler,
                             NodeSamplerInput)

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
DEGS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]
SEED_TIMES = [-1, 0, 3, 7]
KS = [1, 5, 64, 65, 100, -1]
N_COLS = 256
MAX_WAVES = 8192  # kMaxBlocks * kBlock / 64


# ---------------------------------------------------------------------------
# kernel-test graph and its brute-force reference (built once)
# ---------------------------------------------------------------------------
def _kernel_graph():
    g = torch.Generator().manual_seed(1234)
    indptr = torch.zeros(len(DEGS) + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.tensor(DEGS), 0)
    cols = [torch.sort(torch.randint(0, N_COLS, (d,), generator=g)).values
            for d in DEGS]
    indices = torch.cat(cols)
    E = indices.numel()
    return {
        "indptr": indptr, "indices": indices,
        # ids differ from positions, so a position returned as an id fails
        "edge_ids": torch.randperm(E, generator=g) + 1000,
        # ties everywhere; valid edges scattered through the row
        "edge_time": torch.randint(0, 8, (E,), generator=g),
        "node_time": torch.randint(0, 8, (N_COLS,), generator=g),
    }


_CACHE = {}


def kernel_graph():
    if "g" not in _CACHE:
        _CACHE["g"] = _kernel_graph()
    return _CACHE["g"]


def _time_of(g, source, q):
    if source == "edge":
        return int(g["edge_time"][q])
    return int(g["node_time"][g["indices"][q]])


def brute_valid(g, source, row, t):
    """Valid positions of `row` at time t, in row order."""
    if row < 0 or row >= g["indptr"].numel() - 1:
        return []
    lo, hi = int(g["indptr"][row]), int(g["indptr"][row + 1])
    return [q for q in range(lo, hi) if _time_of(g, source, q) <= t]


def brute_last(g, source, valid, cnt):
    order = sorted(valid, key=lambda q: (_time_of(g, source, q), q),
                   reverse=True)
    return order[:cnt]


def combos():
    """(row, time) of the 40 base slots: every row at every seed time."""
    return [(r, t) for r in range(len(DEGS)) for t in SEED_TIMES]


def reference(source):
    """Per base slot: valid positions; shared by all tests, never changed."""
    key = ("ref", source)
    if key not in _CACHE:
        g = kernel_graph()
        _CACHE[key] = [brute_valid(g, source, r, t) for r, t in combos()]
    return _CACHE[key]


def call(g, dev, source, seeds, times, k, with_edge, last):
    d = torch.device(dev)
    out = _C.sample_neighbors_temporal(
        g["indptr"].to(d), g["indices"].to(d), seeds.to(d), times.to(d), k,
        edge_ids=g["edge_ids"].to(d) if with_edge else None,
        edge_time=g["edge_time"].to(d) if source == "edge" else None,
        node_time=g["node_time"].to(d) if source == "node" else None,
        with_edge=with_edge, last=last)
    nbrs, num, eids = out
    assert nbrs.device.type == d.type
    return nbrs.cpu(), num.cpu(), (eids.cpu() if eids is not None else None)


def check_against_brute(g, source, valids, k, with_edge, last, nbrs, num,
                        eids):
    """valids: per-slot valid position lists.  Exact where the contract is
    deterministic; valid + distinct + exact count where it is a draw."""
    kk = math.inf if k < 0 else k
    exp_num = [int(min(kk, len(v))) for v in valids]
    assert num.tolist() == exp_num
    assert nbrs.numel() == sum(exp_num)
    assert (eids is not None) == with_edge
    if with_edge:
        assert eids.numel() == sum(exp_num)
    off = 0
    for v, cnt in zip(valids, exp_num):
        got_n = nbrs[off:off + cnt].tolist()
        got_e = eids[off:off + cnt].tolist() if with_edge else None
        if last or len(v) <= kk:
            pos = brute_last(g, source, v, cnt) if last else v
            assert got_n == g["indices"][pos].tolist()
            if with_edge:
                assert got_e == g["edge_ids"][pos].tolist()
        else:
            if with_edge:
                by_id = {int(g["edge_ids"][q]): q for q in v}
                assert len(set(got_e)) == cnt  # distinct within the slot
                for e, n in zip(got_e, got_n):
                    assert e in by_id  # a valid edge of this row
                    assert n == int(g["indices"][by_id[e]])
            else:
                ok_cols = set(g["indices"][v].tolist())
                assert all(n in ok_cols for n in got_n)
        off += cnt


# ---------------------------------------------------------------------------
# feistel_perm_inv host twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", [0, 0x9E3779B97F4A7C15, 2 ** 64 - 1])
def test_feistel_perm_inv_roundtrip(key):
    for n in list(range(1, 301)) + [2 ** 20 + 3]:
        j = torch.arange(n)
        y = _C.feistel_perm_host(key, j, n, False)
        assert int(y.min()) >= 0 and int(y.max()) < n
        assert torch.equal(_C.feistel_perm_host(key, y, n, True), j), n
        # and the other way round: perm(perm_inv(y)) == y
        x = _C.feistel_perm_host(key, j, n, True)
        assert torch.equal(_C.feistel_perm_host(key, x, n, False), j), n


# ---------------------------------------------------------------------------
# one-hop op vs brute force (CPU twin here, HIP kernels on the GPU)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("last", [False, True], ids=["uniform", "last"])
@pytest.mark.parametrize("with_edge", [True, False], ids=["eid", "noeid"])
@pytest.mark.parametrize("source", ["edge", "node"])
@pytest.mark.parametrize("dev", DEVICES)
def test_one_hop_vs_brute_force(dev, source, with_edge, last):
    g = kernel_graph()
    valids = reference(source)
    seeds = torch.tensor([r for r, _ in combos()])
    times = torch.tensor([t for _, t in combos()])
    _C.manual_seed(3)
    for k in KS:
        nbrs, num, eids = call(g, dev, source, seeds, times, k, with_edge,
                               last)
        check_against_brute(g, source, valids, k, with_edge, last, nbrs,
                            num, eids)
        if dev != "cpu" and (last or k < 0):
            # deterministic outputs equal the CPU twin element for element
            c_nbrs, c_num, c_eids = call(g, "cpu", source, seeds, times, k,
                                         with_edge, last)
            assert torch.equal(nbrs, c_nbrs) and torch.equal(num, c_num)
            if with_edge:
                assert torch.equal(eids, c_eids)


@pytest.mark.parametrize("dev", DEVICES)
def test_p_le_k_matches_cpu_twin(dev):
    """'uniform' slots with p <= k are deterministic: compare them with the
    CPU twin element for element at a k where other slots do draw."""
    g = kernel_graph()
    seeds = torch.tensor([r for r, _ in combos()])
    times = torch.tensor([t for _, t in combos()])
    k = 64
    a = call(g, dev, "edge", seeds, times, k, True, False)
    b = call(g, "cpu", "edge", seeds, times, k, True, False)
    assert torch.equal(a[1], b[1])
    off = 0
    for v, cnt in zip(reference("edge"), a[1].tolist()):
        if len(v) <= k:
            assert torch.equal(a[0][off:off + cnt], b[0][off:off + cnt])
            assert torch.equal(a[2][off:off + cnt], b[2][off:off + cnt])
        off += cnt


@pytest.mark.parametrize("source", ["edge", "node"])
@pytest.mark.parametrize("dev", DEVICES)
def test_same_node_different_times(dev, source):
    g = kernel_graph()
    row = len(DEGS) - 1
    seeds = torch.tensor([row, row, row])
    times = torch.tensor([0, 7, 3])
    nbrs, num, eids = call(g, dev, source, seeds, times, -1, True, False)
    valids = [brute_valid(g, source, row, int(t)) for t in times]
    assert len({len(v) for v in valids}) == 3  # the three sets do differ
    check_against_brute(g, source, valids, -1, True, False, nbrs, num, eids)


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("dev", DEVICES)
def test_out_of_range_seeds(dev, last):
    g = kernel_graph()
    seeds = torch.tensor([-1, len(DEGS), 3, 10 ** 12, -2 ** 40])
    times = torch.full((5,), 7)
    nbrs, num, eids = call(g, dev, "edge", seeds, times, 5, True, last)
    assert num.tolist() == [0, 0, 5, 0, 0]
    assert nbrs.numel() == 5 and eids.numel() == 5


@pytest.mark.parametrize("dev", DEVICES)
def test_empty_inputs(dev):
    g = kernel_graph()
    e = torch.empty(0, dtype=torch.long)
    nbrs, num, eids = call(g, dev, "edge", e, e, 5, True, False)
    assert nbrs.numel() == 0 and num.numel() == 0 and eids.numel() == 0
    # zero total: every slot before all times
    seeds = torch.arange(len(DEGS))
    nbrs, num, eids = call(g, dev, "node", seeds,
                           torch.full_like(seeds, -1), 5, True, True)
    assert nbrs.numel() == 0 and eids.numel() == 0
    assert num.tolist() == [0] * len(DEGS)


@pytest.mark.parametrize("source", ["edge", "node"])
@pytest.mark.parametrize("dev", DEVICES)
def test_grid_stride(dev, source):
    """More seeds than waves launched: the waves stride over the seeds."""
    g = kernel_graph()
    n = 2 * MAX_WAVES + 5
    base = combos()
    valids40 = reference(source)
    sel = [i % len(base) for i in range(n)]
    seeds = torch.tensor([base[c][0] for c in sel])
    times = torch.tensor([base[c][1] for c in sel])
    exp_all = [g["edge_ids"][v] for v in valids40]
    exp_last = [g["edge_ids"][brute_last(g, source, v, min(5, len(v)))]
                for v in valids40]
    # k < 0: p <= k everywhere, fully deterministic
    nbrs, num, eids = call(g, dev, source, seeds, times, -1, True, False)
    assert num.tolist() == [len(valids40[c]) for c in sel]
    assert torch.equal(eids, torch.cat([exp_all[c] for c in sel]))
    # 'last', k = 5
    nbrs, num, eids = call(g, dev, source, seeds, times, 5, True, True)
    assert num.tolist() == [min(5, len(valids40[c])) for c in sel]
    assert torch.equal(eids, torch.cat([exp_last[c] for c in sel]))
    # 'uniform', k = 5: counts exact, every output a valid edge of its row
    _C.manual_seed(11)
    nbrs, num, eids = call(g, dev, source, seeds, times, 5, True, False)
    assert num.tolist() == [min(5, len(valids40[c])) for c in sel]
    off = torch.zeros(n + 1, dtype=torch.long)
    off[1:] = torch.cumsum(num, 0)
    slot = torch.repeat_interleave(torch.arange(n), num)
    ok = torch.zeros(len(base), int(g["edge_ids"].max()) + 1,
                     dtype=torch.bool)
    for c, v in enumerate(valids40):
        ok[c, g["edge_ids"][v]] = True
    assert bool(ok[torch.tensor(sel)[slot], eids].all())
    # distinct within a slot: sort (slot, eid) pairs, no equal neighbours
    key = torch.sort(slot * (ok.size(1) + 1) + eids).values
    assert bool((key[1:] != key[:-1]).all())


def _half_valid_row():
    """The degree-200 row with exactly 100 scattered valid edges at t=0."""
    g = dict(kernel_graph())
    row = len(DEGS) - 1
    lo = int(g["indptr"][row])
    gen = torch.Generator().manual_seed(99)
    valid_pos = torch.randperm(200, generator=gen)[:100] + lo
    et = torch.ones_like(g["edge_time"])
    et[valid_pos] = 0
    g["edge_time"] = et
    return g, row, valid_pos


@pytest.mark.parametrize("dev", DEVICES)
def test_uniformity_and_slot_independence(dev):
    g, row, valid_pos = _half_valid_row()
    n, k, p = 20000, 10, 100
    seeds = torch.full((n,), row)
    times = torch.zeros(n, dtype=torch.long)
    _C.manual_seed(7)
    nbrs, num, eids = call(g, dev, "edge", seeds, times, k, True, False)
    assert num.tolist() == [k] * n
    valid_ids = g["edge_ids"][valid_pos]
    hits = torch.bincount(eids, minlength=int(g["edge_ids"].max()) + 1)
    # no invalid edge ever appears
    assert int(hits.sum()) == int(hits[valid_ids].sum()) == n * k
    q = k / p
    bound = 6 * math.sqrt(n * q * (1 - q))
    assert bound < 255
    c = hits[valid_ids].double()
    print("hit counts: min %d max %d (mean %d, bound +-%.1f)"
          % (c.min(), c.max(), n * q, bound))
    assert bool(((c - n * q).abs() <= bound).all())
    # distinct within a slot
    per = torch.sort(eids.view(n, k), dim=1).values
    assert bool((per[:, 1:] != per[:, :-1]).all())
    # the key belongs to the slot: adjacent slots of the same node draw
    # independently (two draws coincide with probability 1 / C(100, 10))
    differ = (per[1:] != per[:-1]).any(dim=1).double().mean()
    assert float(differ) >= 0.99


# ---------------------------------------------------------------------------
# argument checks: every one raises before any launch
# ---------------------------------------------------------------------------
def _args(dev="cpu"):
    g = kernel_graph()
    d = torch.device(dev)
    seeds = torch.tensor([3, 4], device=d)
    return dict(
        indptr=g["indptr"].to(d), indices=g["indices"].to(d), seeds=seeds,
        seed_time=torch.tensor([3, 3], device=d), k=5,
        edge_ids=g["edge_ids"].to(d), edge_time=g["edge_time"].to(d),
        node_time=None, with_edge=True, last=False)


BAD = {
    "both_sources": lambda a: a.update(
        node_time=kernel_graph()["node_time"].to(a["indptr"].device)),
    "no_source": lambda a: a.update(edge_time=None),
    "seed_time_len": lambda a: a.update(seed_time=a["seed_time"][:1]),
    "edge_time_len": lambda a: a.update(edge_time=a["edge_time"][:-1]),
    "node_time_short": lambda a: a.update(
        edge_time=None,
        node_time=torch.zeros(len(DEGS) - 1, dtype=torch.long,
                              device=a["indptr"].device)),
    "with_edge_no_ids": lambda a: a.update(edge_ids=None),
    "seed_time_int32": lambda a: a.update(
        seed_time=a["seed_time"].to(torch.int32)),
    "edge_time_float": lambda a: a.update(
        edge_time=a["edge_time"].double()),
    "seeds_2d": lambda a: a.update(seeds=a["seeds"].view(1, 2)),
    "edge_time_strided": lambda a: a.update(
        edge_time=torch.stack([a["edge_time"], a["edge_time"]], 1)[:, 0]),
    "seed_time_strided": lambda a: a.update(
        seed_time=torch.zeros(4, dtype=torch.long,
                              device=a["indptr"].device)[::2]),
}


@pytest.mark.parametrize("bad", sorted(BAD))
@pytest.mark.parametrize("dev", DEVICES)
def test_argument_checks(dev, bad):
    a = _args(dev)
    _C.sample_neighbors_temporal(**a)  # the unmodified call is fine
    BAD[bad](a)
    with pytest.raises(RuntimeError):
        _C.sample_neighbors_temporal(**a)


@pytest.mark.gpu
def test_argument_check_device_mismatch():
    a = _args("cuda")
    a["seed_time"] = a["seed_time"].cpu()
    with pytest.raises(RuntimeError):
        _C.sample_neighbors_temporal(**a)
    a = _args("cpu")
    a["edge_time"] = a["edge_time"].cuda()
    with pytest.raises(RuntimeError):
        _C.sample_neighbors_temporal(**a)


# ---------------------------------------------------------------------------
# Topology(edge_times=)
# ---------------------------------------------------------------------------
def _coo(n=50, e=400, seed=5):
    g = torch.Generator().manual_seed(seed)
    row = torch.randint(0, n, (e,), generator=g)
    col = torch.randint(0, n, (e,), generator=g)
    t = torch.randint(0, 1000, (e,), generator=g)
    return n, row, col, t


@pytest.mark.parametrize("layout", ["CSR", "CSC"])
def test_topology_edge_times_coo(layout):
    n, row, col, t = _coo()
    topo = Topology(torch.stack([row, col]), layout=layout, num_nodes=n,
                    edge_times=t)
    assert topo.edge_times.dtype == torch.long
    assert torch.equal(topo.edge_times, t[topo.edge_ids])
    # and the edges themselves went with them
    r, c, eid = topo.to_coo()
    src, dst = (r, c) if layout == "CSR" else (c, r)
    assert torch.equal(row[eid], src) and torch.equal(col[eid], dst)


def _unsorted_csr():
    n, row, col, t = _coo(seed=6)
    order = torch.argsort(row, stable=True)  # rows grouped, columns not
    indptr = torch.zeros(n + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return n, indptr, col[order], t[order], row[order]


def test_topology_edge_times_unsorted_passthrough():
    n, indptr, indices, t, rows = _unsorted_csr()
    topo = Topology((indptr, indices), input_layout="CSR", layout="CSR",
                    edge_times=t)
    assert not torch.equal(topo.indices, indices)  # it did get sorted
    assert torch.equal(topo.edge_times, t[topo.edge_ids])
    assert torch.equal(topo.indices, indices[topo.edge_ids])


def test_topology_edge_times_csr_to_csc():
    n, indptr, indices, t, rows = _unsorted_csr()
    topo = Topology((indptr, indices), input_layout="CSR", layout="CSC",
                    num_nodes=n, edge_times=t)
    assert torch.equal(topo.edge_times, t[topo.edge_ids])
    r, c, eid = topo.to_coo()  # CSC: r = input column, c = input row
    assert torch.equal(indices[eid], r) and torch.equal(rows[eid], c)


def test_topology_without_times_unchanged():
    n, row, col, t = _coo()
    topo = Topology(torch.stack([row, col]), num_nodes=n)
    assert topo.edge_times is None
    from glt_amd.utils.topo import coo_to_csc, coo_to_csr

    assert len(coo_to_csr(row, col, num_rows=n)) == 4
    assert len(coo_to_csc(row, col, num_cols=n)) == 4
    assert len(coo_to_csr(row, col, num_rows=n, edge_time=t)) == 5


def test_graph_edge_times_cpu_and_pickle():
    import pickle

    n, row, col, t = _coo()
    g = Graph(Topology(torch.stack([row, col]), num_nodes=n, edge_times=t),
              "CPU")
    assert torch.equal(g.edge_times, t[g.edge_ids])
    g2 = pickle.loads(pickle.dumps(g))
    assert torch.equal(g2.edge_times, g.edge_times)


def test_node_sampler_input_carries_time():
    inp = NodeSamplerInput(torch.arange(6), None, torch.arange(6) * 3)
    sub = inp[torch.tensor([4, 1])]
    assert sub.time.tolist() == [12, 3] and sub.node.tolist() == [4, 1]
    assert inp.to("cpu").time is not None
    assert inp.share_memory().time.is_shared()
    assert NodeSamplerInput(torch.arange(3))[0:2].time is None


# ---------------------------------------------------------------------------
# NeighborSampler / NeighborLoader
# ---------------------------------------------------------------------------
N_NODES, N_EDGES, T_MAX = 200, 2000, 50


def _temporal_data():
    if "data" not in _CACHE:
        g = torch.Generator().manual_seed(42)
        _CACHE["data"] = {
            "src": torch.randint(0, N_NODES, (N_EDGES,), generator=g),
            "dst": torch.randint(0, N_NODES, (N_EDGES,), generator=g),
            "etime": torch.randint(0, T_MAX, (N_EDGES,), generator=g),
            "ntime": torch.randint(0, T_MAX, (N_NODES,), generator=g),
            # a repeated seed (3) stays two slots
            "seeds": torch.tensor([3, 7, 3, 11, 199, 0, 57, 3, 120, 64]),
            "stime": torch.randint(0, T_MAX, (10,), generator=g),
        }
    return _CACHE["data"]


def _dataset(mode):
    d = _temporal_data()
    ds = Dataset()
    ds.init_graph(edge_index=torch.stack([d["src"], d["dst"]]),
                  graph_mode=mode, num_nodes=N_NODES, device=0,
                  edge_times=d["etime"])
    ds.init_node_times(d["ntime"])
    ds.init_node_features(
        torch.arange(N_NODES, dtype=torch.float32).unsqueeze(1).repeat(1, 4),
        split_ratio=1.0 if mode != "CPU" else 0.0, device=0,
        with_gpu=mode != "CPU")
    ds.init_node_labels(torch.arange(N_NODES))
    return ds


def _edge_ok_time(d, time_attr, e, nbr):
    return int(d["etime"][e]) if time_attr == "edge" else int(
        d["ntime"][nbr])


def _bfs(d, time_attr, seed, t, hops):
    """Time-respecting BFS node set of one slot."""
    adj = _CACHE.setdefault("adj", {})
    if not adj:
        for e in range(N_EDGES):
            adj.setdefault(int(d["src"][e]), []).append(
                (int(d["dst"][e]), e))
    seen, frontier = {seed}, {seed}
    for _ in range(hops):
        nxt = set()
        for u in frontier:
            for v, e in adj.get(u, []):
                if _edge_ok_time(d, time_attr, e, v) <= t:
                    nxt.add(v)
        frontier = nxt - seen
        seen |= nxt
    return seen


def check_output(out, d, time_attr, seeds, stime, fanout):
    node = out.node.cpu()
    row, col, edge = out.row.cpu(), out.col.cpu(), out.edge.cpu()
    si = out.metadata["seed_index"].cpu()
    st = out.metadata["seed_time"].cpu()
    n_seed = seeds.numel()
    assert torch.equal(out.batch.cpu(), seeds)  # in order, no dedup
    assert torch.equal(st, stime)
    assert si.numel() == node.numel()
    assert torch.equal(si[:n_seed], torch.arange(n_seed))
    assert torch.equal(node[:n_seed], seeds)
    pairs = si * N_NODES + node
    assert torch.unique(pairs).numel() == pairs.numel()
    assert sum(out.num_sampled_nodes) == node.numel()
    assert sum(out.num_sampled_edges) == row.numel() == edge.numel()
    # every edge stays inside one tree, exists, and respects the seed time
    assert torch.equal(si[row], si[col])
    assert torch.equal(d["src"][edge], node[row])
    assert torch.equal(d["dst"][edge], node[col])
    etime = d["etime"][edge] if time_attr == "edge" else d["ntime"][node[col]]
    assert bool((etime <= st[si[row]]).all())
    # rows keep the sorted-by-target order of the non-temporal path
    e0 = 0
    for ne in out.num_sampled_edges:
        r = row[e0:e0 + ne]
        assert bool((r[1:] >= r[:-1]).all())
        e0 += ne
    if all(k < 0 for k in fanout):
        for s in range(n_seed):
            got = set(node[si == s].tolist())
            assert got == _bfs(d, time_attr, int(seeds[s]), int(stime[s]),
                               len(fanout))
    else:
        deg = torch.bincount(row, minlength=node.numel())
        assert int(deg.max()) <= max(fanout)


def _sampler(ds, time_attr, strategy, fanout, dev=None):
    return NeighborSampler(
        ds.get_graph(), fanout, device=dev, with_edge=True,
        time_attr=time_attr, node_time=ds.get_node_time(),
        temporal_strategy=strategy, seed=5)


MODES = ["CPU", pytest.param("CUDA", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("fanout", [[5, 5], [-1, -1]], ids=["k5", "all"])
@pytest.mark.parametrize("strategy", ["uniform", "last"])
@pytest.mark.parametrize("time_attr", ["node", "edge"])
@pytest.mark.parametrize("mode", MODES)
def test_sampler_multihop(mode, time_attr, strategy, fanout):
    d = _temporal_data()
    s = _sampler(_dataset(mode), time_attr, strategy, fanout)
    assert not s.use_deferred
    out = s.sample_from_nodes(
        NodeSamplerInput(d["seeds"], None, d["stime"]))
    check_output(out, d, time_attr, d["seeds"], d["stime"], fanout)
    assert not s._deferred_pool  # the deferred path did not run


@pytest.mark.parametrize("mode", MODES)
def test_sampler_last_is_most_recent(mode):
    """'last' with fan-out k keeps, per source, the k latest valid edges."""
    d = _temporal_data()
    s = _sampler(_dataset(mode), "edge", "last", [3])
    out = s.sample_from_nodes(
        NodeSamplerInput(d["seeds"], None, d["stime"]))
    row, edge = out.row.cpu(), out.edge.cpu()
    for slot in range(d["seeds"].numel()):
        u, t = int(d["seeds"][slot]), int(d["stime"][slot])
        cand = [(int(d["etime"][e]), e) for e in range(N_EDGES)
                if int(d["src"][e]) == u and int(d["etime"][e]) <= t]
        got = sorted(int(d["etime"][e]) for e in edge[row == slot])
        want = sorted(tt for tt, _ in cand)[-3:]
        assert got == want


@pytest.mark.parametrize("mode", MODES)
def test_sampler_node_default_seed_time(mode):
    """time_attr='node' without seed times: the seeds' own node time."""
    d = _temporal_data()
    s = _sampler(_dataset(mode), "node", "uniform", [-1, -1])
    out = s.sample_from_nodes(NodeSamplerInput(d["seeds"]))
    check_output(out, d, "node", d["seeds"], d["ntime"][d["seeds"]],
                 [-1, -1])
    s = _sampler(_dataset(mode), "edge", "uniform", [2])
    with pytest.raises(ValueError):
        s.sample_from_nodes(NodeSamplerInput(d["seeds"]))


@pytest.mark.parametrize("mode", MODES)
def test_loader_shuffle_keeps_times_aligned(mode):
    ds = _dataset(mode)
    seeds = torch.arange(0, N_NODES, 2)
    dev = torch.device("cuda", 0) if mode != "CPU" else None
    loader = NeighborLoader(ds, [4, 4], input_nodes=seeds, batch_size=16,
                            shuffle=True, with_edge=True, time_attr="node",
                            input_time=3 * seeds, device=dev, to_device=dev)
    seen = []
    for data in loader:
        assert torch.equal(data.seed_time.cpu(), 3 * data.batch.cpu())
        assert data.x.size(0) == data.node.numel()
        assert torch.equal(data.x[:, 0].cpu().long(), data.node.cpu())
        assert torch.equal(data.y.cpu(), data.batch.cpu())
        si = data.seed_index.cpu()
        assert torch.equal(si[data.edge_index[0].cpu()],
                           si[data.edge_index[1].cpu()])
        seen.append(data.batch.cpu())
    seen = torch.cat(seen)
    assert torch.equal(torch.sort(seen).values, seeds)
    assert not torch.equal(seen, seeds)  # it did shuffle


@pytest.mark.parametrize("mode", MODES)
def test_loader_drop_last_and_pyg_v1(mode):
    d = _temporal_data()
    ds = _dataset(mode)
    seeds = torch.arange(50)
    times = torch.randint(0, T_MAX, (50,),
                          generator=torch.Generator().manual_seed(1))
    loader = NeighborLoader(ds, [3, 3], input_nodes=seeds, batch_size=16,
                            drop_last=True, time_attr="edge",
                            input_time=times, with_edge=True)
    assert len(loader) == 3
    batches = list(loader)
    assert len(batches) == 3
    for i, data in enumerate(batches):
        assert torch.equal(data.batch.cpu(), seeds[16 * i:16 * i + 16])
        assert torch.equal(data.seed_time.cpu(), times[16 * i:16 * i + 16])
    v1 = NeighborLoader(ds, [3, 3], input_nodes=seeds, batch_size=16,
                        time_attr="edge", input_time=times, as_pyg_v1=True)
    bs, n_id, adjs = next(iter(v1))
    assert bs == 16 and len(adjs) == 2
    assert adjs[-1].size[1] == 16


def test_temporal_not_implemented_and_bad_config():
    d = _temporal_data()
    ds = _dataset("CPU")
    g = ds.get_graph()
    with pytest.raises(NotImplementedError):
        NeighborSampler({("a", "to", "a"): g}, [2], time_attr="edge")
    with pytest.raises(NotImplementedError):
        NeighborSampler(g, [2], time_attr="edge", with_weight=True)
    s = NeighborSampler(g, [2], time_attr="edge")
    with pytest.raises(NotImplementedError):
        s.sample_from_edges(EdgeSamplerInput(d["src"][:4], d["dst"][:4]))
    with pytest.raises(NotImplementedError):
        Dataset().init_graph(
            edge_index={("a", "to", "a"): torch.stack([d["src"], d["dst"]])},
            graph_mode="CPU", edge_times=d["etime"])
    from glt_amd.distributed import DistNeighborSampler

    with pytest.raises(NotImplementedError):
        DistNeighborSampler(None, [2], time_attr="edge")
    with pytest.raises(ValueError):
        NeighborSampler(g, [2], time_attr="node")  # no node_time
    with pytest.raises(ValueError):
        NeighborSampler(g, [2], time_attr="when")
    with pytest.raises(ValueError):
        NeighborSampler(g, [2], time_attr="edge", temporal_strategy="first")
    plain = Dataset().init_graph(
        edge_index=torch.stack([d["src"], d["dst"]]), graph_mode="CPU",
        num_nodes=N_NODES)
    with pytest.raises(ValueError):
        NeighborSampler(plain.get_graph(), [2], time_attr="edge")
    with pytest.raises(ValueError):
        NeighborLoader(ds, [2], input_nodes=torch.arange(8),
                       time_attr="edge")  # 'edge' needs input_time
    with pytest.raises(ValueError):
        NeighborLoader(ds, [2], input_nodes=torch.arange(8),
                       time_attr="edge", input_time=torch.arange(7))


def test_non_temporal_sampler_untouched():
    """Without time_attr the sampler deduplicates seeds as before and adds
    no temporal metadata."""
    ds = _dataset("CPU")
    s = NeighborSampler(ds.get_graph(), [3, 3], seed=1)
    out = s.sample_from_nodes(NodeSamplerInput(torch.tensor([3, 7, 3])))
    assert out.batch.tolist() == [3, 7]
    assert "seed_index" not in out.metadata


# -- GPU only ---------------------------------------------------------------
@pytest.mark.gpu
def test_zero_copy_graph():
    d = _temporal_data()
    ds = _dataset("ZERO_COPY")
    for time_attr in ("edge", "node"):
        s = _sampler(ds, time_attr, "uniform", [-1, -1])
        out = s.sample_from_nodes(
            NodeSamplerInput(d["seeds"], None, d["stime"]))
        check_output(out, d, time_attr, d["seeds"], d["stime"], [-1, -1])


@pytest.mark.gpu
def test_deferred_path_only_without_time_attr():
    ds = _dataset("CUDA")
    dev = torch.device("cuda", 0)
    seeds = torch.arange(32)
    temporal = NeighborLoader(ds, [2, 2], input_nodes=seeds, batch_size=8,
                              device=dev, time_attr="node")
    assert not temporal.sampler.use_deferred
    next(iter(temporal))
    assert len(temporal.sampler._deferred_pool) == 0
    plain = NeighborLoader(ds, [2, 2], input_nodes=seeds, batch_size=8,
                           device=dev)
    assert plain.sampler.use_deferred
    next(iter(plain))
    assert len(plain.sampler._deferred_pool) > 0


@pytest.mark.gpu
def test_loader_prefetch():
    ds = _dataset("CUDA")
    dev = torch.device("cuda", 0)
    seeds = torch.arange(64)
    loader = NeighborLoader(ds, [3, 3], input_nodes=seeds, batch_size=16,
                            shuffle=True, time_attr="node",
                            input_time=3 * seeds, device=dev, to_device=dev,
                            prefetch=2)
    n = 0
    for data in loader:
        assert torch.equal(data.seed_time.cpu(), 3 * data.batch.cpu())
        n += data.batch.numel()
    loader.shutdown()
    assert n == 64


@pytest.mark.gpu
def test_graph_edge_times_device_placement():
    n, row, col, t = _coo()
    topo = Topology(torch.stack([row, col]), num_nodes=n, edge_times=t)
    for mode in ("CUDA", "ZERO_COPY"):
        g = Graph(topo, mode, 0)
        assert g.edge_times.is_cuda
        assert torch.equal(g.edge_times.cpu(), topo.edge_times)

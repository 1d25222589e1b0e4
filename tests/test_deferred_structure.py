"""Structure of a deferred-sync batch (_C.DeferredSampler.run) against a
plain-torch oracle on the CPU.

Nothing here is a recorded value: every expectation is computed from the
returned tensors and the CSR.  Edge ids are a permutation + 1000, so each
sampled edge names its CSR position and the checks can speak about
positions: rows are the frontier's local ids repeated min(deg, k) times,
a row with deg <= k holds all its edges in row order, a row with deg > k
holds k distinct ones, cols lead back to the CSR neighbour, and a hop's new
nodes are the first-occurrence uniques of its neighbours not seen before.
"""
import pytest
import torch

from glt_amd import _C

pytestmark = pytest.mark.gpu


def _graph(degs, seed):
    gen = torch.Generator().manual_seed(seed)
    n = len(degs)
    degs = torch.as_tensor(degs, dtype=torch.long)
    indptr = torch.zeros(n + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(degs, 0)
    E = int(indptr[-1])
    return {"n": n, "degs": degs, "indptr": indptr,
            "indices": torch.randint(0, n, (E,), generator=gen),
            "edge_ids": torch.randperm(E, generator=gen) + 1000,
            "row_of_pos": torch.repeat_interleave(torch.arange(n), degs)}


def _small_graph():
    """50 nodes.  Against fan-out 3: node 0 has degree 0, node 3 degree 2
    (< k), node 7 degree 3 (== k), node 11 degree 8 (> k); against the
    second hop's fan-out 2 the degrees 1, 2 and >= 3 all occur."""
    degs = [(4 + v % 5) for v in range(50)]
    degs[0], degs[3], degs[7], degs[11] = 0, 2, 3, 8
    for v in (5, 19, 33):
        degs[v] = 1
    for v in (9, 21, 40):
        degs[v] = 2
    return _graph(degs, 101)


def _big_graph():
    """3000 nodes of degree 0..9; the tests draw their seeds from the first
    300, so both hops still find nodes that no seed named."""
    gen = torch.Generator().manual_seed(7)
    return _graph(torch.randint(0, 10, (3000,), generator=gen).tolist(), 102)


def _run(ds, g, seeds, L):
    d = torch.device("cuda")
    parts, rows, cols, eids, stats = ds.run(
        g["indptr"].to(d), g["indices"].to(d), g["edge_ids"].to(d),
        seeds.to(d))
    s = stats.cpu().tolist()
    n_new, e_tot = s[:L + 1], s[L + 1:]
    # the tensors are views of the sampler's buffers: copy before a next run
    return {"stats": s,
            "parts": [parts[i][:n_new[i]].cpu() for i in range(L + 1)],
            "rows": [rows[h][:e_tot[h]].cpu() for h in range(L)],
            "cols": [cols[h][:e_tot[h]].cpu() for h in range(L)],
            "eids": [eids[h][:e_tot[h]].cpu() for h in range(L)]}


def _first_unique(ids, seen):
    out = []
    for v in ids:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _check(g, seeds, fanout, got):
    L = len(fanout)
    stats, parts = got["stats"], got["parts"]
    assert len(stats) == 2 * L + 1
    seen = set()
    assert parts[0].tolist() == _first_unique(seeds.tolist(), seen)
    assert stats[0] == parts[0].numel()
    node = torch.cat(parts)
    pos_of_eid = torch.full((g["edge_ids"].numel() + 1000,), -1,
                            dtype=torch.long)
    pos_of_eid[g["edge_ids"]] = torch.arange(g["edge_ids"].numel())
    base = 0
    for h, k in enumerate(fanout):
        frontier = parts[h]
        ids = base + torch.arange(frontier.numel())
        deg = g["degs"][frontier]
        cnt = deg.clamp(max=k)
        rows, cols, eids = got["rows"][h], got["cols"][h], got["eids"][h]
        assert stats[L + 1 + h] == int(cnt.sum()) == rows.numel()
        assert torch.equal(rows, torch.repeat_interleave(ids, cnt))
        if rows.numel() > 1:
            assert bool((rows[1:] >= rows[:-1]).all())
        # every sampled edge is a CSR edge of its row and leads to its col
        pos = pos_of_eid[eids]
        assert bool((pos >= 0).all())
        assert torch.equal(g["row_of_pos"][pos], node[rows])
        assert torch.equal(g["indices"][pos], node[cols])
        at = 0
        for v, d, c in zip(frontier.tolist(), deg.tolist(), cnt.tolist()):
            p = pos[at:at + c] - int(g["indptr"][v])
            if d <= k:      # all neighbours, in row order
                assert p.tolist() == list(range(d))
            else:           # k distinct positions of the row
                assert torch.unique(p).numel() == k
                assert int(p.min()) >= 0 and int(p.max()) < d
            at += c
        new = _first_unique(g["indices"][pos].tolist(), seen)
        assert parts[h + 1].tolist() == new
        assert stats[1 + h] == len(new)
        base += frontier.numel()
    assert torch.unique(node).numel() == node.numel()


def test_small_graph_duplicate_seeds_every_degree_class():
    g = _small_graph()
    assert [int(g["degs"][v]) for v in (0, 3, 7, 11)] == [0, 2, 3, 8]
    seeds = torch.tensor([7, 7, 3, 0, 7])
    fanout = [3, 2]
    _C.manual_seed(31)
    got = _run(_C.DeferredSampler(fanout, 1024, 0, True), g, seeds, 2)
    _check(g, seeds, fanout, got)
    assert got["parts"][0].tolist() == [7, 3, 0]
    # the first hop reached rows the second hop samples from
    assert got["rows"][1].numel() > 0


def test_many_duplicate_seeds_across_workgroups():
    g = _big_graph()
    gen = torch.Generator().manual_seed(8)
    seeds = torch.randint(0, 300, (2000,), generator=gen)
    fanout = [4, 3]
    _C.manual_seed(32)
    got = _run(_C.DeferredSampler(fanout, 2048, 0, True), g, seeds, 2)
    _check(g, seeds, fanout, got)
    assert got["rows"][0].numel() > 256      # more than one workgroup
    assert got["parts"][0].numel() <= 300    # duplicates did collide
    assert got["parts"][1].numel() > 0 and got["parts"][2].numel() > 0


def test_one_sampler_two_batches_in_a_row():
    """A table left over from the first batch would number the second
    batch's nodes as already seen."""
    g = _big_graph()
    gen = torch.Generator().manual_seed(9)
    fanout = [4, 3]
    ds = _C.DeferredSampler(fanout, 1024, 0, True)
    _C.manual_seed(33)
    first = torch.randint(0, 300, (700,), generator=gen)
    second = torch.randint(0, 300, (40,), generator=gen)
    _check(g, first, fanout, _run(ds, g, first, 2))
    _check(g, second, fanout, _run(ds, g, second, 2))


def test_same_seed_same_batch():
    g = _big_graph()
    gen = torch.Generator().manual_seed(10)
    seeds = torch.randint(0, 300, (500,), generator=gen)
    fanout = [4, 3]
    ds = _C.DeferredSampler(fanout, 1024, 0, True)
    runs = []
    for _ in range(2):
        _C.manual_seed(34)
        runs.append(_run(ds, g, seeds, 2))
    a, b = runs
    assert a["stats"] == b["stats"]
    for key in ("parts", "rows", "cols", "eids"):
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y)
    assert any(int(d) > 4 for d in g["degs"][a["parts"][0]])  # draws happened

"""Data-path kernels at their branch edges: the non-temporal samplers
(hip_sampler.hip), the inducer / subgraph / stitch kernels (hip_inducer.hip),
the deferred-sync sampler (hip_deferred.hip) and the feature gather
(hip_unified_tensor.hip).

Every reference is a brute-force Python / NumPy / fp64 computation on the
host, built once and never changed.  The shared assertion helpers run
unmarked on the CPU twins (`_C.*` on host tensors) and marked `gpu` on the
HIP kernels.

Fixture: the ladder graph.  One CSR row per degree in DEGS (0..5, the wave
edges 63/64/65, 127..129, 300, and the chunked-CDF sizes 4097 and 10000).
Column ids are scattered over [0, N_NODES), sorted and unique within a row;
a few of them are ladder row ids so that second hops and walks continue.
Edge ids are a permutation + 1000, so a position returned as an id fails.

The statistical bound is the binomial 6-sigma bound, derived, not fitted.
A count c of successes in n independent trials of probability p has mean
n*p and standard deviation sqrt(n*p*(1-p)); a case passes iff every count
holds |c - n*p| <= 6 * sqrt(n*p*(1-p)) (and c == 0 where p == 0).
 - Uniform sampling without replacement: a slot (one seed occurrence) draws
   k of deg edges under its own key, so "edge i is in slot s" is
   Bernoulli(k/deg), independent across slots: n = slots, p = k/deg.
 - Weighted with replacement: every draw is independent, so edge i is hit
   Binomial(slots*k, w_i/W) times.  Weights are small non-negative
   integers: every CDF partial sum is exact in fp32 in any order, and the
   2^-24 grid of u moves a probability by less than 1e-6 sigma.
 - Weighted without replacement (Efraimidis-Spirakis): the first output of
   a slot is the minimum of independent exponentials of rates w_i, which is
   edge i with probability exactly w_i/W: n = slots, p = w_i/W.
The normal tail beyond 6 sigma is 2e-9 per count; where n*p is small the
binomial's upper tail is heavier, so single edges are bounded only where
n*p >= 20 and the light edges of the hub rows are bounded in 16 position
bins (a bin of m edges of probability q each is Binomial(n, m*q)).  Every
statistical test seeds the native RNG, so a run is deterministic.
"""
import math

import numpy as np
import pytest
import torch

import glt_amd
from glt_amd import _C

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
DEGS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 300, 4097, 10000)
WDEGS = tuple(sorted(DEGS + (20,)))  # the weighted cases also need deg 20
N_NODES = 16384
SLOTS = 20000
MAX_THREADS = 2048 * 256  # kMaxBlocks * kBlock: more work grid-strides

_CACHE = {}


# ---------------------------------------------------------------------------
# the ladder graph and its brute-force views (built once per degree list)
# ---------------------------------------------------------------------------
def _build_ladder(degs):
    gen = torch.Generator().manual_seed(20240 + len(degs))
    nr = len(degs)
    indptr = torch.zeros(nr + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    cols = []
    for d in degs:
        m = min(d // 2, 4)  # ladder row ids among the neighbours
        low = torch.randperm(nr, generator=gen)[:m]
        high = torch.randperm(N_NODES - nr, generator=gen)[:d - m] + nr
        cols.append(torch.sort(torch.cat([low, high])).values)
    indices = torch.cat(cols)
    E = indices.numel()
    edge_ids = torch.randperm(E, generator=gen) + 1000
    pos_of_eid = torch.full((E + 1000,), -1, dtype=torch.long)
    pos_of_eid[edge_ids] = torch.arange(E)
    row_of_pos = torch.repeat_interleave(torch.arange(nr), torch.tensor(degs))
    return {"degs": degs, "nr": nr, "indptr": indptr, "indices": indices,
            "edge_ids": edge_ids, "pos_of_eid": pos_of_eid,
            "row_of_pos": row_of_pos, "E": E,
            "row": {d: i for i, d in enumerate(degs)}}


def ladder(degs=DEGS):
    key = ("ladder", degs)
    if key not in _CACHE:
        _CACHE[key] = _build_ladder(degs)
    return _CACHE[key]


def deg_of(g, v):
    return g["degs"][v] if 0 <= v < g["nr"] else 0


def row_cols(g, v):
    lo, hi = int(g["indptr"][v]), int(g["indptr"][v + 1])
    return g["indices"][lo:hi]


def mixed_seeds(g, negatives=True):
    """Every row; repeats; zero-degree rows (row 0) and out-of-range ids
    between live rows; first and last row included."""
    nr, h = g["nr"], g["nr"] // 2
    s = [0, nr - 3, nr, h - 1, h - 1, 0, h, nr + 7, h + 1, 0, 1]
    s += [v for v in range(nr)] + [nr - 1, 5, 4]
    if negatives:
        s[4:4] = [-1]
        s[9:9] = [-(2 ** 40)]
    return torch.tensor(s)


def test_ladder_fixture_self_check():
    for degs in (DEGS, WDEGS):
        g = ladder(degs)
        assert g["indptr"].tolist()[-1] == g["E"] == sum(degs)
        for v, d in enumerate(degs):
            c = row_cols(g, v)
            assert c.numel() == d
            assert bool((c[1:] > c[:-1]).all())  # sorted and unique
            assert d == 0 or (int(c[0]) >= 0 and int(c[-1]) < N_NODES)
        assert not torch.equal(g["edge_ids"], torch.arange(g["E"]))
        assert torch.equal(g["pos_of_eid"][g["edge_ids"]],
                           torch.arange(g["E"]))
        assert not torch.equal(g["indices"], torch.arange(g["E"]))
    s = mixed_seeds(ladder()).tolist()
    assert s[0] == 0 and len(DEGS) - 1 in s and -1 in s and len(DEGS) in s
    assert len(DEGS) + 7 in s


# ---------------------------------------------------------------------------
# the binomial helper
# ---------------------------------------------------------------------------
def sigma_ratio(counts, n, probs):
    """max |c - n p| / sqrt(n p (1 - p)) over the entries with 0 < p < 1;
    inf if an entry with p == 0 was hit or one with p == 1 was missed."""
    c = torch.as_tensor(counts, dtype=torch.double)
    p = torch.as_tensor(probs, dtype=torch.double)
    assert c.shape == p.shape
    if bool((c[p <= 0] != 0).any()) or bool((c[p >= 1] != n).any()):
        return math.inf
    m = (p > 0) & (p < 1)
    if not bool(m.any()):
        return 0.0
    sd = torch.sqrt(n * p[m] * (1 - p[m]))
    return float(((c[m] - n * p[m]).abs() / sd).max())


def assert_binomial(counts, n, probs, what):
    r = sigma_ratio(counts, n, probs)
    print("%s: max |c - np| / sigma = %.2f" % (what, r))
    assert r <= 6.0, (what, r)
    return r


def binned(counts, probs, skip=(), bins=16):
    """Sum counts and probabilities over `bins` position bins, leaving out
    the positions in `skip`."""
    c = torch.as_tensor(counts, dtype=torch.double).clone()
    p = torch.as_tensor(probs, dtype=torch.double).clone()
    for s in skip:
        c[s] = 0
        p[s] = 0
    idx = (torch.arange(c.numel()) * bins) // c.numel()
    return (torch.zeros(bins, dtype=torch.double).index_add_(0, idx, c),
            torch.zeros(bins, dtype=torch.double).index_add_(0, idx, p))


def test_binomial_helper_rejects_emulated_defects():
    """The check must pass true draws and fail the two ways a wave-kernel
    CDF search can go wrong: every draw on the row's last edge, and a CDF
    shifted by one position."""
    gen = torch.Generator().manual_seed(5)
    for deg, k in ((20, 5), (64, 5), (64, 63)):
        w = (torch.arange(deg) % 7).double()
        p = w / w.sum()
        n = SLOTS * k
        true = torch.bincount(
            torch.multinomial(p, n, replacement=True, generator=gen),
            minlength=deg)
        assert sigma_ratio(true, n, p) <= 6.0
        last = torch.zeros(deg)
        last[deg - 1] = n
        assert sigma_ratio(last, n, p) > 6.0
        shifted = torch.bincount(
            torch.multinomial(torch.roll(p, 1), n, replacement=True,
                              generator=gen), minlength=deg)
        assert sigma_ratio(shifted, n, p) > 6.0
        # and through the bins used for the hub rows
        bc, bp = binned(last, p)
        assert sigma_ratio(bc, n, bp) > 6.0
        bc, bp = binned(true, p)
        assert sigma_ratio(bc, n, bp) <= 6.0


# ---------------------------------------------------------------------------
# one-hop call + the exact checks shared by uniform and weighted sampling
# ---------------------------------------------------------------------------
def one_hop(g, dev, seeds, k, with_edge=True, weights=None, replace=True):
    d = torch.device(dev)
    nbrs, num, eids = _C.sample_neighbors(
        g["indptr"].to(d), g["indices"].to(d), seeds.to(d), k,
        edge_ids=g["edge_ids"].to(d) if with_edge else None,
        edge_weights=weights.to(d) if weights is not None else None,
        with_edge=with_edge, weighted=weights is not None, replace=replace)
    assert nbrs.device.type == d.type
    assert (eids is not None) == with_edge
    return nbrs.cpu(), num.cpu(), (eids.cpu() if with_edge else None)


def check_one_hop(g, seeds, k, nbrs, num, eids, distinct=True):
    """Counts, and per slot: the row in order where deg <= k, else k members
    of the row (distinct unless drawn with replacement) whose edge ids are
    the ids of the positions holding them."""
    kk = math.inf if k < 0 else k
    exp = [int(min(kk, deg_of(g, v))) for v in seeds.tolist()]
    assert num.tolist() == exp
    assert nbrs.numel() == sum(exp)
    if eids is not None:
        assert eids.numel() == sum(exp)
    off = 0
    for v, cnt in zip(seeds.tolist(), exp):
        if cnt == 0:
            continue
        lo = int(g["indptr"][v])
        got = nbrs[off:off + cnt]
        if deg_of(g, v) <= kk:
            assert torch.equal(got, g["indices"][lo:lo + cnt])
            if eids is not None:
                assert torch.equal(eids[off:off + cnt],
                                   g["edge_ids"][lo:lo + cnt])
        else:
            cols = row_cols(g, v)
            at = torch.searchsorted(cols, got).clamp(max=cols.numel() - 1)
            assert torch.equal(cols[at], got)  # members of the row
            if distinct:
                assert torch.unique(got).numel() == cnt
            if eids is not None:
                # columns are unique in a row: the position is determined
                assert torch.equal(eids[off:off + cnt],
                                   g["edge_ids"][lo + at])
        off += cnt


def row_hits(g, v, eids):
    """Hit count per position of row v from returned edge ids."""
    lo = int(g["indptr"][v])
    pos = g["pos_of_eid"][eids] - lo
    assert int(pos.min()) >= 0 and int(pos.max()) < deg_of(g, v)
    return torch.bincount(pos, minlength=deg_of(g, v))


# ---------------------------------------------------------------------------
# uniform sampling
# ---------------------------------------------------------------------------
KS = [1, 2, 5, 63, 64, 65, 128, -1]


@pytest.mark.parametrize("with_edge", [True, False], ids=["eid", "noeid"])
@pytest.mark.parametrize("dev", DEVICES)
def test_uniform_exact(dev, with_edge):
    """deg == k and deg == k + 1 are both covered: k = 4 against the rows of
    degree 4 and 5, k = 64 against the rows of degree 64 and 65."""
    g = ladder()
    seeds = mixed_seeds(g)
    glt_amd.seed_everything(21)
    for k in KS + [4]:
        nbrs, num, eids = one_hop(g, dev, seeds, k, with_edge)
        check_one_hop(g, seeds, k, nbrs, num, eids)


@pytest.mark.gpu
@pytest.mark.parametrize("with_edge", [True, False], ids=["eid", "noeid"])
def test_uniform_staged_pair_equals_one_call(with_edge):
    g = ladder()
    d = torch.device("cuda")
    seeds = mixed_seeds(g)
    ip, ix, ei = g["indptr"].to(d), g["indices"].to(d), g["edge_ids"].to(d)
    sd = seeds.to(d)
    for k in KS:
        glt_amd.seed_everything(22)
        nbrs, num, eids = one_hop(g, "cuda", seeds, k, with_edge)
        glt_amd.seed_everything(22)
        counts, offsets = _C.sample_neighbors_offsets(ip, sd, k)
        assert torch.equal(counts.cpu(), num)
        exp_off = torch.zeros(seeds.numel() + 1, dtype=torch.long)
        exp_off[1:] = torch.cumsum(num, 0)  # exclusive cumsum of the counts
        assert torch.equal(offsets.cpu(), exp_off)
        n2, e2 = _C.sample_neighbors_gather(
            ip, ix, sd, k, offsets, int(exp_off[-1]),
            edge_ids=ei if with_edge else None, with_edge=with_edge)
        assert torch.equal(n2.cpu(), nbrs)
        if with_edge:
            assert torch.equal(e2.cpu(), eids)
        else:
            assert e2 is None


@pytest.mark.parametrize("dev", DEVICES)
def test_uniform_grid_stride(dev):
    """8200 copies of the degree-65 row: 533000 outputs > 524288 threads."""
    g = ladder()
    v = g["row"][65]
    n = 8200
    assert n * 65 > MAX_THREADS
    seeds = torch.full((n,), v)
    nbrs, num, eids = one_hop(g, dev, seeds, 65)
    lo = int(g["indptr"][v])
    assert num.tolist() == [65] * n
    assert torch.equal(nbrs, g["indices"][lo:lo + 65].repeat(n))
    assert torch.equal(eids, g["edge_ids"][lo:lo + 65].repeat(n))
    glt_amd.seed_everything(23)
    nbrs, num, eids = one_hop(g, dev, seeds, 64)
    assert num.tolist() == [64] * n
    pos = g["pos_of_eid"][eids]
    assert int(pos.min()) >= lo and int(pos.max()) < lo + 65
    assert torch.equal(g["indices"][pos], nbrs)
    per = torch.sort(pos.view(n, 64), dim=1).values
    assert bool((per[:, 1:] != per[:, :-1]).all())


UNIFORM_CASES = [(2, 1), (3, 1), (3, 2), (4, 1), (5, 2), (65, 10),
                 (300, 10)]


@pytest.mark.parametrize("deg,k", UNIFORM_CASES)
@pytest.mark.parametrize("dev", DEVICES)
def test_uniform_marginals(dev, deg, k):
    """Inclusion of an edge in a slot is Bernoulli(k/deg) and slots have
    independent keys, so over R = 20000 slots of one row each edge's hit
    count c holds |c - R p| <= 6 sqrt(R p (1 - p)), p = k/deg (module
    docstring).  The CPU twin draws by Floyd's algorithm under a per-slot
    generator: the same marginals, so the same bound."""
    g = ladder()
    v = g["row"][deg]
    seeds = torch.full((SLOTS,), v)
    glt_amd.seed_everything(24)
    nbrs, num, eids = one_hop(g, dev, seeds, k)
    assert num.tolist() == [k] * SLOTS
    hits = row_hits(g, v, eids)
    assert_binomial(hits, SLOTS, torch.full((deg,), k / deg),
                    "uniform %s deg=%d k=%d" % (dev, deg, k))
    per = torch.sort(eids.view(SLOTS, k), dim=1).values
    if k > 1:
        assert bool((per[:, 1:] != per[:, :-1]).all())
    if (deg, k) == (65, 10):
        # two slots coincide with probability 1 / C(65, 10)
        differ = (per[1:] != per[:-1]).any(dim=1).double().mean()
        assert float(differ) >= 0.99


# ---------------------------------------------------------------------------
# deferred-sync sampler (GPU only: it has no CPU twin)
# ---------------------------------------------------------------------------
def _deferred(g, seeds, fanout, cap):
    d = torch.device("cuda")
    ds = _C.DeferredSampler(list(fanout), cap, 0, True)
    parts, rows, cols, eids, stats = ds.run(
        g["indptr"].to(d), g["indices"].to(d), g["edge_ids"].to(d),
        seeds.to(d))
    s = stats.cpu().tolist()
    L = len(fanout)
    n_new, e_tot = s[:L + 1], s[L + 1:]
    return ([parts[i][:n_new[i]].cpu() for i in range(L + 1)],
            [rows[h][:e_tot[h]].cpu() for h in range(L)],
            [cols[h][:e_tot[h]].cpu() for h in range(L)],
            [eids[h][:e_tot[h]].cpu() for h in range(L)])


def _classic(g, seeds, fanout):
    d = torch.device("cuda")
    ip, ix, ei = g["indptr"].to(d), g["indices"].to(d), g["edge_ids"].to(d)
    ind = _C.DeviceInducer(64)
    srcs = ind.init_node(seeds.to(d))
    nodes, rows, cols, eids = [srcs.cpu()], [], [], []
    for k in fanout:
        nbrs, num, e = _C.sample_neighbors(ip, ix, srcs, k, edge_ids=ei,
                                           with_edge=True)
        srcs, r, c = ind.induce_next(srcs, nbrs, num)
        nodes.append(srcs.cpu())
        rows.append(r.cpu())
        cols.append(c.cpu())
        eids.append(e.cpu())
    return nodes, rows, cols, eids


def _deferred_seeds(g):
    """The rows of degree 0..5, the last row, repeats and out-of-range ids;
    never -1 (the table's empty mark).  The other rows are left to be
    reached through the ladder ids among the neighbours."""
    nr = g["nr"]
    return torch.tensor([0, nr - 1, nr, 2, 2, 1, nr + 7, 3, 4, 0, 5, 3])


def test_deferred_seeds_reach_a_second_hop():
    for degs in (DEGS, tuple(d for d in DEGS if d <= 65)):
        g = ladder(degs)
        seeds = set(_deferred_seeds(g).tolist())
        reached = {c for v in (2, 3, 4, 5) for c in row_cols(g, v).tolist()}
        assert any(deg_of(g, c) > 0 for c in reached - seeds)


@pytest.mark.gpu
def test_deferred_full_fanout_equals_classic():
    """Fan-out [65, 65] over rows of degree <= 65 takes every edge, so the
    deferred path equals the classic path tensor for tensor."""
    g = ladder(tuple(d for d in DEGS if d <= 65))
    seeds = _deferred_seeds(g)
    got = _deferred(g, seeds, [65, 65], 16)
    want = _classic(g, seeds, [65, 65])
    for a, b in zip(got, want):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert got[1][1].numel() > 0  # the second hop did sample


@pytest.mark.gpu
def test_deferred_structure_over_all_rows():
    g = ladder()
    seeds = _deferred_seeds(g)
    glt_amd.seed_everything(25)
    parts, rows, cols, eids = _deferred(g, seeds, [5, 5], 16)
    node = torch.cat(parts)
    # seeds first, in first-occurrence order; no duplicate node
    first = list(dict.fromkeys(seeds.tolist()))
    assert parts[0].tolist() == first
    assert torch.unique(node).numel() == node.numel()
    row, col, eid = torch.cat(rows), torch.cat(cols), torch.cat(eids)
    # every edge exists in the graph through its edge id
    pos = g["pos_of_eid"][eid]
    assert int(pos.min()) >= 0
    assert torch.equal(g["row_of_pos"][pos], node[row])
    assert torch.equal(g["indices"][pos], node[col])
    assert torch.unique(eid).numel() == eid.numel()
    # per-source counts: min(deg, 5) for every expanded node, 0 for the rest
    n_src = parts[0].numel() + parts[1].numel()
    want = [min(deg_of(g, v), 5) for v in node[:n_src].tolist()]
    want += [0] * parts[2].numel()
    assert torch.bincount(row, minlength=node.numel()).tolist() == want
    # hop h's rows are hop h's frontier
    assert int(rows[0].max()) < parts[0].numel()
    assert int(rows[1].min()) >= parts[0].numel()


# ---------------------------------------------------------------------------
# weighted sampling
# ---------------------------------------------------------------------------
def ramp(deg):
    """w_i = i % 7: zero-weight edges at the front and scattered."""
    return (torch.arange(deg) % 7).float()


def heavy(deg, at):
    """The hub test's weights: one edge holds half of the mass."""
    w = torch.ones(deg)
    w[at] = float(deg - 1)
    return w


def weights_with(g, rows_w):
    w = torch.ones(g["E"])
    for v, rw in rows_w.items():
        lo = int(g["indptr"][v])
        assert rw.numel() == deg_of(g, v)
        w[lo:lo + rw.numel()] = rw
    return w


def _replace_hits(dev, deg, k, rw):
    """20000 slots of the row of degree `deg` with row weights rw: the hit
    count per position, the probabilities and the number of draws."""
    g = ladder(WDEGS)
    v = g["row"][deg]
    w = weights_with(g, {v: rw})
    seeds = torch.full((SLOTS,), v)
    glt_amd.seed_everything(26)
    nbrs, num, eids = one_hop(g, dev, seeds, k, weights=w)
    assert num.tolist() == [k] * SLOTS
    assert torch.equal(g["indices"][g["pos_of_eid"][eids]], nbrs)
    hits = row_hits(g, v, eids)
    assert int(hits[rw == 0].sum()) == 0  # a zero-weight edge is never hit
    return hits, rw.double() / rw.double().sum(), SLOTS * k


WAVE_CASES = [(2, 1), (3, 2), (20, 5), (63, 1), (64, 5), (64, 63)]


@pytest.mark.parametrize("kind", ["uniform", "ramp"])
@pytest.mark.parametrize("deg,k", WAVE_CASES)
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_replace_small_rows(dev, deg, k, kind):
    """Rows with k < deg <= 64 (the wave kernel on the GPU).  Edge i is hit
    Binomial(20000 k, w_i / W) times (module docstring)."""
    rw = torch.ones(deg) if kind == "uniform" else ramp(deg)
    hits, p, n = _replace_hits(dev, deg, k, rw)
    assert_binomial(hits, n, p,
                    "replace %s deg=%d k=%d %s" % (dev, deg, k, kind))


# (deg, k, heavy position): 65 is the first row the wave kernel leaves; 300
# needs a second scan batch (nch = 300 > 256); 4097 is the first chunked size
# (cs = 2, a last chunk of one edge, which is the heavy one); 10000 has cs = 3.
BLOCK_CASES = [(65, 5, 21), (300, 4, 100), (4097, 4, 4096),
               (10000, 4, 3333)]


@pytest.mark.parametrize("deg,k,at", BLOCK_CASES)
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_replace_large_rows(dev, deg, k, at):
    """Heavy edge (weight deg - 1, half of the mass) at a position that is
    not the first, deg - 1 light edges of weight 1.  n = 20000 k draws.
    The heavy edge is Binomial(n, 1/2).  A light edge has probability
    q = 1 / (2 (deg - 1)); for deg = 10000, n q = 4, too few for a normal
    bound on one edge, so the light edges are summed over 16 position bins,
    each Binomial(n, m q) for its m light edges (n m q >= 2400).  Rows whose
    single light edges expect n q >= 20 hits are bounded per edge as well."""
    what = "replace %s deg=%d k=%d heavy@%d" % (dev, deg, k, at)
    hits, p, n = _replace_hits(dev, deg, k, heavy(deg, at))
    assert_binomial(hits[at:at + 1], n, p[at:at + 1], what + " heavy edge")
    bc, bp = binned(hits, p, skip=(at,))
    assert_binomial(bc, n, bp, what + " 16 bins of light edges")
    if n / (2 * (deg - 1)) >= 20:
        assert_binomial(hits, n, p, what + " per edge")


@pytest.mark.parametrize("with_edge", [True, False], ids=["eid", "noeid"])
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_replace_mixed_rows(dev, with_edge):
    """Seeds cycle through degrees 0, 3, 64, 65, 300 with k = 5: on the GPU
    every row belongs to exactly one of the wave and the block kernel."""
    g = ladder(WDEGS)
    rows = [g["row"][d] for d in (0, 3, 64, 65, 300)]
    w = weights_with(g, {g["row"][64]: ramp(64), g["row"][65]: ramp(65),
                         g["row"][300]: ramp(300)})
    seeds = torch.tensor(rows).repeat(SLOTS)
    k = 5
    glt_amd.seed_everything(27)
    nbrs, num, eids = one_hop(g, dev, seeds, k, with_edge, weights=w)
    cnt = [0, 3, 5, 5, 5]
    assert num.view(SLOTS, 5).eq(torch.tensor(cnt)).all()
    nb = nbrs.view(SLOTS, sum(cnt))
    eb = eids.view(SLOTS, sum(cnt)) if with_edge else None
    off = 0
    for v, c in zip(rows, cnt):
        if c == 0:
            continue
        cols = row_cols(g, v)
        lo = int(g["indptr"][v])
        got = nb[:, off:off + c]
        if deg_of(g, v) <= k:  # copied in order
            assert bool((got == cols).all())
            if with_edge:
                assert bool((eb[:, off:off + c]
                             == g["edge_ids"][lo:lo + c]).all())
        else:
            at = torch.searchsorted(cols, got.reshape(-1)).clamp(
                max=cols.numel() - 1)
            assert torch.equal(cols[at], got.reshape(-1))  # own row only
            if with_edge:
                assert torch.equal(g["edge_ids"][lo + at],
                                   eb[:, off:off + c].reshape(-1))
            hits = torch.bincount(at, minlength=cols.numel())
            rw = w[lo:lo + cols.numel()].double()
            assert int(hits[rw == 0].sum()) == 0
            if deg_of(g, v) in (64, 65):
                assert_binomial(hits, SLOTS * k, rw / rw.sum(),
                                "mixed %s deg=%d" % (dev, deg_of(g, v)))
        off += c


@pytest.mark.parametrize("replace", [True, False])
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_all_zero_rows(dev, replace):
    g = ladder(WDEGS)
    rows = [g["row"][d] for d in (3, 64, 300)]
    w = weights_with(g, {v: torch.zeros(deg_of(g, v)) for v in rows})
    seeds = torch.tensor(rows).repeat(50)
    glt_amd.seed_everything(28)
    nbrs, num, eids = one_hop(g, dev, seeds, 2, weights=w, replace=replace)
    check_one_hop(g, seeds, 2, nbrs, num, eids, distinct=False)


NOREPLACE_CASES = [(20, 5), (64, 8), (300, 8)]


@pytest.mark.parametrize("deg,k", NOREPLACE_CASES)
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_no_replace(dev, deg, k):
    """Efraimidis-Spirakis: output 0 of a slot is the minimum key, which is
    edge i with probability exactly w_i / W, so over 20000 slots edge i is
    first Binomial(20000, w_i / W) times.  Rows of degree <= 64 go to the
    block kernel here too."""
    g = ladder(WDEGS)
    v = g["row"][deg]
    rw = ramp(deg)
    w = weights_with(g, {v: rw})
    seeds = torch.full((SLOTS,), v)
    glt_amd.seed_everything(29)
    nbrs, num, eids = one_hop(g, dev, seeds, k, weights=w, replace=False)
    assert num.tolist() == [k] * SLOTS
    assert torch.equal(g["indices"][g["pos_of_eid"][eids]], nbrs)
    hits = row_hits(g, v, eids)
    assert int(hits[rw == 0].sum()) == 0  # enough positive edges exist
    per = torch.sort(eids.view(SLOTS, k), dim=1).values
    assert bool((per[:, 1:] != per[:, :-1]).all())  # distinct in a slot
    first = row_hits(g, v, eids.view(SLOTS, k)[:, 0].contiguous())
    assert_binomial(first, SLOTS, rw.double() / rw.double().sum(),
                    "no-replace first %s deg=%d k=%d" % (dev, deg, k))


@pytest.mark.parametrize("deg,npos,k", [(20, 3, 6), (300, 2, 5)])
@pytest.mark.parametrize("dev", DEVICES)
def test_weighted_no_replace_fewer_positive_than_k(dev, deg, npos, k):
    g = ladder(WDEGS)
    v = g["row"][deg]
    rw = torch.zeros(deg)
    where = torch.tensor([1, deg // 2, deg - 1][:npos])
    rw[where] = torch.tensor([3.0, 1.0, 2.0][:npos])
    w = weights_with(g, {v: rw})
    n = 500
    seeds = torch.full((n,), v)
    glt_amd.seed_everything(30)
    nbrs, num, eids = one_hop(g, dev, seeds, k, weights=w, replace=False)
    check_one_hop(g, seeds, k, nbrs, num, eids, distinct=False)
    lo = int(g["indptr"][v])
    pos = (g["pos_of_eid"][eids] - lo).view(n, k)
    head = torch.sort(pos[:, :npos], dim=1).values
    assert bool((head == where).all())  # exactly the positive set


@pytest.mark.gpu
def test_weighted_no_replace_k_limit():
    """k = 257 raises before the sampling kernel is launched.  (The CPU twin
    has no such limit: its selection is a partial sort.)"""
    g = ladder(WDEGS)
    w = torch.ones(g["E"])
    seeds = torch.tensor([g["row"][300]])
    one_hop(g, "cuda", seeds, 256, weights=w, replace=False)
    with pytest.raises(RuntimeError):
        one_hop(g, "cuda", seeds, 257, weights=w, replace=False)


# ---------------------------------------------------------------------------
# negative sampling, random walk, degree, probability
# ---------------------------------------------------------------------------
def _bipartite():
    indptr = torch.arange(0, 101, 10)
    indices = torch.arange(10).repeat(10)
    return indptr, indices


@pytest.mark.parametrize("dev", DEVICES)
def test_negative_sampling(dev):
    g = ladder()
    d = torch.device(dev)
    glt_amd.seed_everything(31)
    neg = _C.sample_negative(g["indptr"].to(d), g["indices"].to(d), N_NODES,
                             4096, 10, False).cpu()
    assert neg.dim() == 2 and neg.size(0) == 2
    # about 5 % of the candidates are edges: rejection does run
    assert 4000 <= neg.size(1) <= 4096
    r, c = neg[0], neg[1]
    assert int(r.min()) >= 0 and int(r.max()) < g["nr"]
    assert int(c.min()) >= 0 and int(c.max()) < N_NODES
    edges = set(zip(g["row_of_pos"].tolist(), g["indices"].tolist()))
    assert not any(pair in edges for pair in zip(r.tolist(), c.tolist()))
    assert torch.unique(r).numel() == g["nr"]
    # complete bipartite block: every trial is exhausted
    ip, ix = _bipartite()
    out = _C.sample_negative(ip.to(d), ix.to(d), 10, 4096, 10, False)
    assert tuple(out.shape) == (2, 0)
    out = _C.sample_negative(ip.to(d), ix.to(d), 10, 4096, 10, True).cpu()
    assert tuple(out.shape) == (2, 4096)
    assert int(out.min()) >= 0 and int(out.max()) < 10


@pytest.mark.parametrize("dev", DEVICES)
def test_random_walk(dev):
    """Node ids >= the number of rows have no row: a walk that reaches one
    stays there, as it does at the zero-degree row."""
    g = ladder()
    d = torch.device(dev)
    ip, ix = g["indptr"].to(d), g["indices"].to(d)
    seeds = torch.cat([torch.arange(g["nr"]),
                       torch.tensor([g["row"][0], g["nr"] + 7, N_NODES])])
    seeds = seeds.repeat(20)
    glt_amd.seed_everything(32)
    walks = _C.random_walk(ip, ix, seeds.to(d), 6).cpu()
    assert tuple(walks.shape) == (seeds.numel(), 7)
    assert torch.equal(walks[:, 0], seeds)
    edges = set(zip(g["row_of_pos"].tolist(), g["indices"].tolist()))
    moved = 0
    for a, b in zip(walks[:, :-1].reshape(-1).tolist(),
                    walks[:, 1:].reshape(-1).tolist()):
        if deg_of(g, a) == 0:
            assert b == a  # dead end or no such row: stays in place
        else:
            assert (a, b) in edges
            moved += 1
    # some walks did take a second step
    assert moved > sum(deg_of(g, v) > 0 for v in seeds.tolist())
    # first step from the degree-4 row: Binomial(20000, 1/4) per neighbour
    v = g["row"][4]
    walks = _C.random_walk(ip, ix, torch.full((SLOTS,), v).to(d), 6).cpu()
    cols = row_cols(g, v)
    at = torch.searchsorted(cols, walks[:, 1].contiguous()).clamp(max=3)
    assert torch.equal(cols[at], walks[:, 1])
    assert_binomial(torch.bincount(at, minlength=4), SLOTS,
                    torch.full((4,), 0.25), "random walk first step " + dev)


@pytest.mark.parametrize("dev", DEVICES)
def test_lookup_degree(dev):
    g = ladder()
    d = torch.device(dev)
    gen = torch.Generator().manual_seed(33)
    n = 600000
    assert n > MAX_THREADS
    ids = torch.randint(-3, g["nr"] + 8, (n,), generator=gen)
    ids[:4] = torch.tensor([0, g["nr"] - 1, g["nr"], -1])
    table = torch.zeros(g["nr"] + 11, dtype=torch.long)
    table[3:3 + g["nr"]] = torch.tensor(g["degs"])
    got = _C.lookup_degree(g["indptr"].to(d), ids.to(d)).cpu()
    assert torch.equal(got, table[ids + 3])


def _prob_graph():
    """400 nodes, k = 5.  Rows 0..49 all point at node 399 (contended
    atomics) and have degree 1, 5 (= k) or 6 (= k + 1); row 50 has degree
    300.  last_prob cycles through {0, 0.25, 0.5, 1}."""
    if "prob" in _CACHE:
        return _CACHE["prob"]
    gen = torch.Generator().manual_seed(34)
    n, k = 400, 5
    degs = [(1, 5, 6)[r % 3] for r in range(50)] + [300] + [0] * (n - 51)
    cols = []
    for r in range(50):
        other = torch.randperm(340, generator=gen)[:degs[r] - 1] + 51
        cols.append(torch.sort(torch.cat([other,
                                          torch.tensor([399])])).values)
    cols.append(torch.sort(torch.randperm(n, generator=gen)[:300]).values)
    indptr = torch.zeros(n + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.tensor(degs), 0)
    indices = torch.cat(cols)
    last = torch.tensor([0.0, 0.25, 0.5, 1.0]).repeat(n // 4)
    # the row order puts every last_prob value on every degree
    nodes = torch.arange(51)
    # fp64: 1 - (1 - p_v) * prod_{u -> v} (1 - min(1, k / deg_u) p_u)
    keep = np.ones(n)
    for u in nodes.tolist():
        pe = min(1.0, k / degs[u]) * float(last[u])
        for v in indices[indptr[u]:indptr[u + 1]].tolist():
            keep[v] *= 1.0 - pe
    ref = torch.from_numpy(1.0 - (1.0 - last.double().numpy()) * keep)
    _CACHE["prob"] = (indptr, indices, last, nodes, k, ref, degs)
    return _CACHE["prob"]


def _prob_err(dev):
    indptr, indices, last, nodes, k, ref, _ = _prob_graph()
    d = torch.device(dev)
    out = _C.cal_nbr_prob(indptr.to(d), indices.to(d), last.to(d),
                          nodes.to(d), k).cpu()
    assert out.dtype == torch.float32 and out.numel() == ref.numel()
    return out, float((out.double() - ref).abs().max())


def test_cal_nbr_prob_cpu_twin():
    """fp32 twin against fp64.  With S the log-sum of a node, the result is
    1 - (1 - p) e^S; an error dS moves it by (1 - p) e^S dS, and e^S |S|
    <= 1/e, so 50 fp32 additions and logs (each <= 2^-23 relative) stay far
    below 1e-5."""
    indptr, indices, last, nodes, k, ref, degs = _prob_graph()
    out, err = _prob_err("cpu")
    print("cal_nbr_prob cpu twin max error %.3g" % err)
    assert err <= 1e-5
    # a source with p_edge == 1 (deg <= k, last_prob 1) forces probability 1
    forced = [u for u in nodes.tolist()
              if degs[u] <= k and float(last[u]) == 1.0]
    assert forced
    assert abs(float(ref[399]) - 1.0) < 1e-12
    assert abs(float(out[399]) - 1.0) <= 1e-6


@pytest.mark.gpu
def test_cal_nbr_prob_gpu():
    """The kernel may use fast-math log / exp and adds in any order: it is
    allowed 4x the CPU twin's measured error plus 1e-6."""
    _, _, _, _, _, ref, _ = _prob_graph()
    _, cpu_err = _prob_err("cpu")
    out, err = _prob_err("cuda")
    tol = 4 * cpu_err + 1e-6
    print("cal_nbr_prob max error: cpu twin %.3g, kernel %.3g (tol %.3g)"
          % (cpu_err, err, tol))
    assert err <= tol
    assert abs(float(out[399]) - 1.0) <= tol  # the p_edge == 1 factor


# ---------------------------------------------------------------------------
# inducer
# ---------------------------------------------------------------------------
def _inducer_script():
    """Seeds and three hops over sparse ids below 2^40 (never -1): duplicate
    seeds; hop 1 and 2 with duplicates inside the hop and ids of earlier
    hops, sized so that a table made for 8 ids grows twice; hop 3 brings
    nothing new.  The reference is a Python dict."""
    if "ind" in _CACHE:
        return _CACHE["ind"]
    gen = torch.Generator().manual_seed(35)
    pool = torch.unique(torch.randint(0, 2 ** 40, (600,), generator=gen))
    pool = pool[torch.randperm(pool.numel(), generator=gen)][:500]
    pool[7] = 2 ** 40 - 1
    pool[8] = 0
    absent = torch.tensor([1, 2 ** 40 - 2, 12345, 2 ** 62])
    assert not bool(torch.isin(absent, pool).any())
    seeds = pool[torch.tensor([0, 1, 2, 0, 3, 1, 4, 5, 6, 7, 8, 9])]
    local = {}

    def insert(ids):
        new = []
        for v in ids.tolist():
            if v not in local:
                local[v] = len(local)
                new.append(v)
        return torch.tensor(new, dtype=torch.long)

    hops = []
    srcs = insert(seeds)
    uniq_seeds = srcs
    for h, (per, lo, hi) in enumerate([(6, 0, 50), (8, 0, 500), (1, 0, 0)]):
        ns = srcs.numel()
        if h < 2:
            nbrs = pool[torch.randint(lo, hi, (ns * per,), generator=gen)]
        else:  # only ids that are already in
            seen = torch.tensor(list(local))
            nbrs = seen[torch.randint(0, seen.numel(), (ns * per,),
                                      generator=gen)]
        num = torch.full((ns,), per)
        new = insert(nbrs)
        rows = torch.tensor([local[v] for v in srcs.tolist()]
                            ).repeat_interleave(per)
        cols = torch.tensor([local[v] for v in nbrs.tolist()])
        hops.append((srcs, nbrs, num, new, rows, cols))
        if h < 2:
            assert 0 < new.numel() < nbrs.numel()  # some new, some not
            srcs = new
        else:
            assert new.numel() == 0
    # 64 slots for the seeds; hop 1 and hop 2 each need more than there are
    c0, c1 = uniq_seeds.numel(), uniq_seeds.numel() + hops[0][3].numel()
    assert 2 * (c0 + hops[0][1].numel()) > 64
    assert 2 * (c1 + hops[1][1].numel()) > 256
    _CACHE["ind"] = (seeds, uniq_seeds, hops, dict(local), absent)
    return _CACHE["ind"]


@pytest.mark.parametrize("dev", DEVICES)
def test_inducer_three_hops(dev):
    """CPUInducer has neither lookup() nor count(): those two are checked on
    the device inducer only."""
    seeds, uniq_seeds, hops, local, absent = _inducer_script()
    d = torch.device(dev)
    ind = _C.CPUInducer(8) if dev == "cpu" else _C.DeviceInducer(8)
    assert torch.equal(ind.init_node(seeds.to(d)).cpu(), uniq_seeds)
    count = uniq_seeds.numel()
    for srcs, nbrs, num, new, rows, cols in hops:
        n, r, c = ind.induce_next(srcs.to(d), nbrs.to(d), num.to(d))
        assert torch.equal(n.cpu(), new)  # first-occurrence order
        assert torch.equal(r.cpu(), rows)
        assert torch.equal(c.cpu(), cols)
        count += new.numel()
        if dev != "cpu":
            assert ind.count() == count
    if dev != "cpu":
        keys = torch.tensor(list(local))
        assert ind.lookup(keys.to(d)).cpu().tolist() == list(local.values())
        assert ind.lookup(absent.to(d)).cpu().tolist() == [-1] * 4


@pytest.mark.gpu
def test_inducer_staged_insert_equals_one_insert():
    seeds, uniq_seeds, hops, _, _ = _inducer_script()
    d = torch.device("cuda")
    a, b = hops[0][1].to(d), hops[1][1].to(d)
    one = _C.DeviceInducer(8)
    one.init_node(seeds.to(d))
    want = one.insert(torch.cat([a, b]))
    two = _C.DeviceInducer(8)
    two.init_node(seeds.to(d))
    two.reserve_incoming(a.numel() + b.numel())
    fa, ra = two.insert_begin(a, 0)
    fb, rb = two.insert_begin(b, a.numel())
    na, nb = int(ra[-1]), int(rb[-1])
    ua = two.insert_commit(a, fa, ra, na)
    ub = two.insert_commit(b, fb, rb, nb)
    assert torch.equal(torch.cat([ua, ub]), want)
    assert two.count() == one.count()
    every = torch.cat([seeds.to(d), a, b])
    assert torch.equal(two.lookup(every), one.lookup(every))
    assert int(two.lookup(every).min()) >= 0


@pytest.mark.parametrize("dev", DEVICES)
def test_inducer_heavy_duplication(dev):
    """600000 ids from 5000 distinct values in one call: grid-stride, and on
    the GPU about 120 threads contend for each slot's first-index minimum."""
    gen = torch.Generator().manual_seed(36)
    vals = torch.unique(torch.randint(0, 2 ** 40, (6000,), generator=gen))
    vals = vals[torch.randperm(vals.numel(), generator=gen)][:5000]
    n = 600000
    assert n > MAX_THREADS
    ids = vals[torch.randint(0, 5000, (n,), generator=gen)]
    u, first = np.unique(ids.numpy(), return_index=True)
    order = np.argsort(first)
    want = torch.from_numpy(u[order])
    d = torch.device(dev)
    ind = _C.CPUInducer(8) if dev == "cpu" else _C.DeviceInducer(8)
    assert torch.equal(ind.init_node(ids.to(d)).cpu(), want)
    # the same through a hop: relabelled columns
    new, rows, cols = ind.induce_next(
        want[:1].to(d), ids.to(d), torch.tensor([n]).to(d))
    assert new.numel() == 0
    assert bool((rows.cpu() == 0).all())
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    want_cols = torch.from_numpy(rank[np.searchsorted(u, ids.numpy())])
    assert torch.equal(cols.cpu(), want_cols)


# ---------------------------------------------------------------------------
# node subgraph
# ---------------------------------------------------------------------------
def _random_graph():
    if "rg" in _CACHE:
        return _CACHE["rg"]
    gen = torch.Generator().manual_seed(37)
    n = 300
    pair = torch.unique(torch.randint(0, n * n, (3100,), generator=gen))
    row, col = pair // n, pair % n  # sorted by (row, col), no duplicates
    indptr = torch.zeros(n + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    eid = torch.randperm(pair.numel(), generator=gen) + 500
    _CACHE["rg"] = (n, indptr, row, col, eid)
    return _CACHE["rg"]


@pytest.mark.parametrize("size", [1, 64, 65, 300])
@pytest.mark.parametrize("dev", DEVICES)
def test_node_subgraph(dev, size):
    n, indptr, row, col, eid = _random_graph()
    assert 2800 <= row.numel() <= 3100
    gen = torch.Generator().manual_seed(38 + size)
    base = torch.randperm(n, generator=gen)[:size]
    # duplicates and an id without a row (never -1)
    nodes = torch.cat([base, base[:max(1, size // 3)],
                       torch.tensor([n + 5]), base[-1:]])
    uniq = list(dict.fromkeys(nodes.tolist()))
    where = {v: i for i, v in enumerate(uniq)}
    id_of = {(r, c): e for r, c, e in
             zip(row.tolist(), col.tolist(), eid.tolist())}
    want = [(u, c) for u in uniq if u < n
            for c in col[indptr[u]:indptr[u + 1]].tolist() if c in where]
    d = torch.device(dev)
    un, r, c, e = _C.node_subgraph(indptr.to(d), col.to(d), nodes.to(d),
                                   edge_ids=eid.to(d), with_edge=True)
    un, r, c, e = un.cpu(), r.cpu(), c.cpu(), e.cpu()
    assert un.tolist() == uniq  # first-occurrence order
    assert list(zip(un[r].tolist(), un[c].tolist())) == want
    assert r.tolist() == [where[a] for a, _ in want]
    assert c.tolist() == [where[b] for _, b in want]
    assert e.tolist() == [id_of[p] for p in want]
    if size == 300:
        assert len(want) == row.numel()
    un2, r2, c2, e2 = _C.node_subgraph(indptr.to(d), col.to(d), nodes.to(d))
    assert e2 is None and torch.equal(r2.cpu(), r) and torch.equal(
        c2.cpu(), c)
    if dev != "cpu":  # the CPU twin's order, tensor for tensor
        t = _C.node_subgraph(indptr, col, nodes, edge_ids=eid,
                             with_edge=True)
        for x, y in zip((un, r, c, e), t):
            assert torch.equal(x, y)


# ---------------------------------------------------------------------------
# stitch
# ---------------------------------------------------------------------------
def _stitch_case(name):
    """Per-seed values first; the expectation is their concatenation in seed
    order.  Partitions hold shuffled (interleaved) seed positions."""
    key = ("stitch", name)
    if key in _CACHE:
        return _CACHE[key]
    gen = torch.Generator().manual_seed(39)
    if name == "grid":
        ns = 9010
        counts = torch.full((ns,), 65)
        counts[9000:] = torch.tensor([0, 1, 5, 64, 65] * 2)
        part_of = torch.zeros(ns, dtype=torch.long)
        part_of[9000:] = 1
        nparts = 2
    else:
        ns = 45
        counts = torch.tensor([0, 1, 5, 64, 65] * 9)
        part_of = torch.randint(0, 2, (ns,), generator=gen) * 2  # 0 or 2
        nparts = 3
        if name == "zero":  # partition 1: some of the zero-count seeds only
            part_of[torch.tensor([0, 10, 20, 25])] = 1
    off = torch.zeros(ns + 1, dtype=torch.long)
    off[1:] = torch.cumsum(counts, 0)
    total = int(off[-1])
    nbrs = torch.randperm(total, generator=gen) + 7
    eids = torch.randperm(total, generator=gen) + 10 ** 6
    idx_l, nbr_l, num_l, eid_l = [], [], [], []
    for p in range(nparts):
        idx = torch.nonzero(part_of == p).view(-1)
        idx = idx[torch.randperm(idx.numel(), generator=gen)]
        pick = torch.cat([torch.arange(int(off[s]), int(off[s + 1]))
                          for s in idx.tolist()] +
                         [torch.empty(0, dtype=torch.long)])
        idx_l.append(idx)
        num_l.append(counts[idx])
        nbr_l.append(nbrs[pick])
        eid_l.append(eids[pick])
    if name == "empty":
        assert idx_l[1].numel() == 0
    if name == "zero":
        assert idx_l[1].numel() == 4 and int(num_l[1].sum()) == 0
    if name == "grid":
        assert nbr_l[0].numel() == 9000 * 65 > MAX_THREADS
    _CACHE[key] = (ns, idx_l, nbr_l, num_l, eid_l, counts, nbrs, eids)
    return _CACHE[key]


@pytest.mark.parametrize("with_edge", [True, False], ids=["eid", "noeid"])
@pytest.mark.parametrize("name", ["empty", "zero", "grid"])
@pytest.mark.parametrize("dev", DEVICES)
def test_stitch(dev, name, with_edge):
    ns, idx_l, nbr_l, num_l, eid_l, counts, nbrs, eids = _stitch_case(name)
    d = torch.device(dev)
    mv = lambda ts: [t.to(d) for t in ts]  # noqa: E731
    out = _C.stitch_sample_results(ns, mv(idx_l), mv(nbr_l), mv(num_l),
                                   mv(eid_l) if with_edge else [])
    assert torch.equal(out[1].cpu(), counts)
    assert torch.equal(out[0].cpu(), nbrs)
    if with_edge:
        assert torch.equal(out[2].cpu(), eids)
    else:
        assert out[2] is None
    if dev != "cpu":
        twin = _C.stitch_sample_results(ns, idx_l, nbr_l, num_l,
                                        eid_l if with_edge else [])
        assert torch.equal(out[0].cpu(), twin[0])
        assert torch.equal(out[1].cpu(), twin[1])
        if with_edge:
            assert torch.equal(out[2].cpu(), twin[2])


# ---------------------------------------------------------------------------
# unified feature store (GPU only: the gather has no CPU twin)
# ---------------------------------------------------------------------------
SEG_ROWS = [7, 64, 1, 129, 50]
# row bytes = 0 mod 16, 8 mod 16, 4 mod 8, 2 mod 4 and odd, per dtype
GATHER_CASES = [
    (torch.float32, 4), (torch.float32, 2), (torch.float32, 1),
    (torch.float32, 33), (torch.bfloat16, 1), (torch.bfloat16, 3),
    (torch.bfloat16, 4), (torch.bfloat16, 8), (torch.float16, 2),
    (torch.float16, 5), (torch.uint8, 1), (torch.uint8, 7),
    (torch.uint8, 16), (torch.int64, 1), (torch.int64, 2),
    (torch.int64, 3),
]


def _bits(shape, dtype, gen):
    """Random bit patterns of `dtype` (compared as bytes: NaNs included)."""
    nbytes = torch.empty(0, dtype=dtype).element_size()
    raw = torch.randint(0, 256, (shape[0], shape[1] * nbytes),
                        dtype=torch.uint8, generator=gen)
    return raw.view(dtype)


def _store(full, seg_rows, mapped=()):
    store = _C.UnifiedFeatureStore(0)
    keep, lo = [], 0
    for i, n in enumerate(seg_rows):
        part = full[lo:lo + n].contiguous()
        if i in mapped:
            keep.append(part)
            store.append(_C.host_mapped_view(part, 0))
        else:
            store.append(part.cuda())
        lo += n
    return store, keep


def _edge_rows(seg_rows, n_random, gen):
    starts = np.concatenate([[0], np.cumsum(seg_rows)])
    edge = [int(s) for s in starts[:-1]] + [int(s) - 1 for s in starts[1:]]
    total = int(starts[-1])
    rnd = torch.randint(0, total, (n_random,), generator=gen).tolist()
    rows = edge + edge[::-1] + rnd + [0, 0, total - 1, total - 1]
    return torch.tensor(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,dim", GATHER_CASES,
                         ids=lambda v: str(v).replace("torch.", ""))
def test_feature_gather_widths(dtype, dim):
    gen = torch.Generator().manual_seed(40)
    full = _bits((sum(SEG_ROWS), dim), dtype, gen)
    store, keep = _store(full, SEG_ROWS, mapped=(3,))
    assert store.rows() == sum(SEG_ROWS) and store.dim() == dim
    rows = _edge_rows(SEG_ROWS, 300, gen)
    out = store.gather(rows.cuda())
    assert out.dtype == dtype and tuple(out.shape) == (rows.numel(), dim)
    assert torch.equal(out.cpu().view(torch.uint8),
                       full[rows].view(torch.uint8))
    empty = store.gather(torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(empty.shape) == (0, dim) and empty.dtype == dtype


@pytest.mark.gpu
def test_feature_gather_grid_stride():
    gen = torch.Generator().manual_seed(41)
    segs = [1000, 1, 1099]
    full = torch.randn(sum(segs), 516, generator=gen)
    store, _ = _store(full, segs)
    assert 4200 * (516 * 4 // 16) > MAX_THREADS
    rows = _edge_rows(segs, 4200 - 16, gen)
    assert rows.numel() == 4200
    assert torch.equal(store.gather(rows.cuda()).cpu(), full[rows])


@pytest.mark.gpu
def test_feature_store_argument_checks():
    full = torch.arange(17 * 3, dtype=torch.float32).view(17, 3)
    store, _ = _store(full[:16], [1] * 16)  # 16 segments are accepted
    rows = torch.tensor([15, 0, 7, 15], device="cuda")
    assert torch.equal(store.gather(rows).cpu(), full[rows.cpu()])
    with pytest.raises(RuntimeError):
        store.append(full[16:].cuda())  # the 17th
    store = _C.UnifiedFeatureStore(0)
    store.append(full[:4].cuda())
    bad = [full[4:8].cuda().half(),              # dtype
           full[4:8, :2].contiguous().cuda(),    # width
           full.cuda()[4:12:2],                  # non-contiguous
           full[4:8],                            # host tensor
           full[4].cuda()]                       # 1-D
    for seg in bad:
        with pytest.raises(RuntimeError):
            store.append(seg)
    assert store.rows() == 4
    with pytest.raises(RuntimeError):
        store.gather(torch.tensor([0]))  # host indices
    with pytest.raises(RuntimeError):
        _C.UnifiedFeatureStore(0).gather(rows)  # empty store

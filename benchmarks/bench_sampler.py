#!/usr/bin/env python3
"""Neighbor-sampling micro-benchmark: sampled edges/sec (M).

Mirrors the reference harness metric (reference
benchmarks/api/bench_sampler.py:46-53) on a synthetic ogbn-products-shaped
graph: 3-hop [15,10,5], batch 1024, reporting sampled edges per second.
Modes: CUDA (HBM CSR) and ZERO_COPY (pinned-host UVA CSR).

--temporal {node,edge} switches to temporal sampling.  It prints two more
JSON lines before the multi-hop one: the one-hop temporal call
(_C.sample_neighbors_temporal) against the non-temporal _C.sample_neighbors
on the same graph, seeds and k (= the first fan-out), alternated over
--rounds rounds, with the scan's effective bandwidth.  Times are uniform in
[0, 100); --valid-frac sets the seed time so that about that share of the
edges is valid.
"""
import argparse
import json
import time

import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def one_hop_compare(args, graph, sampler, n, t_seed, has_gpu):
    """One-hop temporal call vs the non-temporal call, alternated."""
    from glt_amd import _C

    g = graph
    dev = g.indptr.device
    k = int(args.fanout.split(",")[0])
    by_edge = args.temporal == "edge"
    last = args.temporal_strategy == "last"
    gen = torch.Generator().manual_seed(1)
    seeds = torch.randint(0, n, (args.batch_size,), generator=gen).to(dev)
    stime = torch.full_like(seeds, t_seed)
    deg_sum = int((g.indptr[seeds + 1] - g.indptr[seeds]).sum())

    def plain():
        return _C.sample_neighbors(g.indptr, g.indices, seeds, k)

    def temporal():
        return _C.sample_neighbors_temporal(
            g.indptr, g.indices, seeds, stime, k,
            edge_time=g.edge_times if by_edge else None,
            node_time=None if by_edge else sampler.node_time, last=last)

    def timed(fn):
        if has_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        edges = 0
        for _ in range(args.iters):
            edges += fn()[0].numel()
        if has_gpu:
            torch.cuda.synchronize()
        return edges, time.perf_counter() - t0

    for fn in (plain, temporal):
        for _ in range(3):
            fn()
    rounds = {"plain": [], "temporal": []}
    for _ in range(args.rounds):  # alternated: same build, same session
        for name, fn in (("plain", plain), ("temporal", temporal)):
            edges, dt = timed(fn)
            rounds[name].append((edges, dt))
    # Bytes the temporal call has to move.  The row is walked twice (count
    # pass + select pass; 'last' walks it once per emitted edge after the
    # count pass, which this formula does not model).  Per edge and pass:
    # 8 B time ('edge') or 8 B column id + 8 B node-time gather ('node').
    # Per emitted edge: 8 B store, plus an 8 B column gather with 'edge'.
    # Per seed: seed, time, 2 x indptr, valid_num, count, 2 x offsets.
    out_edges = rounds["temporal"][0][0] // args.iters
    per_edge = 8 if by_edge else 16
    nbytes = (2 * deg_sum * per_edge + out_edges * (16 if by_edge else 8)
              + seeds.numel() * 64)
    for name, rs in rounds.items():
        rates = [e / dt / 1e6 for e, dt in rs]
        rec = {
            "metric": f"one_hop_{name}_edges_per_sec_M",
            "rounds": [round(r, 2) for r in rates],
            "ms_per_call": [round(dt / args.iters * 1e3, 4) for _, dt in rs],
            "k": k, "batch_size": args.batch_size, "deg_sum": deg_sum,
            "edges_per_call": rs[0][0] // args.iters,
        }
        if name == "temporal":
            rec.update({
                "temporal": args.temporal,
                "strategy": args.temporal_strategy,
                "valid_frac": args.valid_frac,
                "scan_bytes_per_call": nbytes,
                "effective_GBps": [round(nbytes * args.iters / dt / 1e9, 2)
                                   for _, dt in rs],
            })
        print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_449_029)
    ap.add_argument("--edges", type=int, default=61_859_140)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--fanout", type=str, default="15,10,5")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--mode", type=str, default="CUDA",
                    choices=["CUDA", "ZERO_COPY", "CPU"])
    ap.add_argument("--with-features", action="store_true")
    ap.add_argument("--feat-dim", type=int, default=100)
    ap.add_argument("--temporal", type=str, default=None,
                    choices=["node", "edge"])
    ap.add_argument("--temporal-strategy", type=str, default="uniform",
                    choices=["uniform", "last"])
    ap.add_argument("--valid-frac", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import glt_amd
    from glt_amd.data import Feature, Graph, Topology
    from glt_amd.sampler import NeighborSampler, NodeSamplerInput

    glt_amd.seed_everything(0)
    has_gpu = torch.cuda.is_available()
    if not has_gpu:
        args.nodes, args.edges, args.iters = 20_000, 400_000, 5
        args.mode = "CPU"
    dev = torch.device("cuda", 0) if has_gpu and args.mode != "CPU" \
        else torch.device("cpu")
    gen = torch.device("cuda", 0) if has_gpu else torch.device("cpu")

    n, e = args.nodes, args.edges
    src = torch.randint(0, n, (e,), device=gen)
    dst = torch.randint(0, n, (e,), device=gen)
    row = torch.cat([src, dst])
    col = torch.cat([dst, src])
    perm = torch.argsort(row)
    row_s, col_s = row[perm], col[perm]
    indptr = torch.zeros(n + 1, dtype=torch.long, device=gen)
    torch.cumsum(torch.bincount(row_s, minlength=n), 0, out=indptr[1:])

    topo = Topology.__new__(Topology)
    topo.layout = "CSR"
    topo.edge_ids = None
    topo.edge_weights = None
    etime = ntime = None
    if args.temporal == "edge":
        etime = torch.randint(0, 100, (col_s.numel(),), device=gen)
    elif args.temporal == "node":
        ntime = torch.randint(0, 100, (n,), device=gen)
    topo.edge_times = (etime if args.mode == "CUDA" or etime is None
                       else etime.cpu())
    if args.mode == "CUDA":
        topo.indptr, topo.indices = indptr, col_s
    else:
        topo.indptr, topo.indices = indptr.cpu(), col_s.cpu()
    graph = Graph(topo, mode=args.mode, device=0 if has_gpu else None)
    if args.mode == "CUDA":
        graph._indptr, graph._indices = indptr, col_s
        graph._edge_ids = graph._edge_weights = None
        graph._edge_times = etime
        graph._lazy_done = True

    fanout = [int(x) for x in args.fanout.split(",")]
    sampler = NeighborSampler(graph, fanout, device=dev,
                              time_attr=args.temporal, node_time=ntime,
                              temporal_strategy=args.temporal_strategy)
    # seed time: times are uniform in [0, 100), so t = 100 * frac - 1 makes
    # about `frac` of the edges valid
    t_seed = int(round(100 * args.valid_frac)) - 1
    if args.temporal is not None:
        one_hop_compare(args, graph, sampler, n, t_seed, has_gpu)
    feature = None
    if args.with_features:
        feats = torch.randn(n, args.feat_dim)
        feature = Feature(feats, split_ratio=1.0 if args.mode == "CUDA"
                          else 0.0, device=0, with_gpu=has_gpu)

    def seed_input(seeds):
        if args.temporal is None:
            return NodeSamplerInput(seeds)
        return NodeSamplerInput(seeds, None, torch.full_like(seeds, t_seed))

    total_edges = 0
    total_nodes = 0
    # warmup
    for _ in range(3):
        seeds = torch.randint(0, n, (args.batch_size,), device=dev)
        out = sampler.sample_from_nodes(seed_input(seeds))
    if has_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        seeds = torch.randint(0, n, (args.batch_size,), device=dev)
        out = sampler.sample_from_nodes(seed_input(seeds))
        total_edges += out.row.numel()
        total_nodes += out.node.numel()
        if feature is not None:
            x = feature[out.node]
    if has_gpu:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({
        "metric": "sampled_edges_per_sec_M",
        "value": round(total_edges / dt / 1e6, 2),
        "mode": args.mode,
        "temporal": args.temporal,
        "with_features": args.with_features,
        "batches_per_sec": round(args.iters / dt, 2),
        "avg_edges_per_batch": total_edges // args.iters,
        "avg_nodes_per_batch": total_nodes // args.iters,
        "ms_per_batch": round(dt / args.iters * 1e3, 3),
    }))


if __name__ == "__main__":
    main()

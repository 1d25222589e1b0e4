#!/usr/bin/env python3
"""glt_amd flagship benchmark — GraphSAGE on synthetic ogbn-products.

Metric (BASELINE.json): end-to-end training step throughput (batches/sec,
reported with epoch-time equivalent) for GraphSAGE on an ogbn-products-shaped
graph: 2,449,029 nodes, 61,859,140 undirected edges (123.7M directed),
100-dim float features, 47 classes, fan-out [15,10,5], batch 1024 — synthetic
(random) graph + random-init weights since this environment has no network.

A "step" = sample 3-hop neighborhood of 1024 seeds + gather features +
forward + backward + optimizer step.  Weak scaling: each rank owns a full
graph replica and processes its own batches; DDP all-reduce over RCCL/xGMI.

Run:  python bench.py --gpus N --steps K --warmup W
  --dump-outputs DIR  also writes the last timed step's results as .npy
                      (same arguments => same inputs, run to run)
  --full              reserved for secondary measurements (none today)
Multi-GPU (driver):  python -m torch.distributed.run --nnodes=1
  --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch
import torch.distributed as dist
import torch.nn.functional as F


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=None,
                   help="timed steps (default 300; 5 without a GPU)")
    p.add_argument("--warmup", type=int, default=None,
                   help="untimed warmup steps (default 20; 2 without a GPU)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step computed (loss, seed-node logits, seed ids, "
                        "labels) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement or check. "
                        "This benchmark has none besides the headline "
                        "figure, so the flag currently adds nothing")
    p.add_argument("--batch-size", type=int, default=1024)
    p.add_argument("--fanout", type=str, default="15,10,5")
    p.add_argument("--nodes", type=int, default=2_449_029)
    p.add_argument("--edges", type=int, default=61_859_140)
    p.add_argument("--feat-dim", type=int, default=100)
    p.add_argument("--classes", type=int, default=47)
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--graph-mode", type=str, default="CUDA",
                   choices=["CUDA", "ZERO_COPY", "CPU"])
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--prefetch", type=int, default=3)
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["fp32", "bf16"],
                   help="default bf16: features stored bf16, bf16 MFMA "
                        "GEMMs/segment kernels with fp32 accumulation + "
                        "fp32 master params (manual mixed precision; "
                        "accuracy-gated by the SBM tests). --dtype fp32 "
                        "reproduces the reference-precision path")
    p.add_argument("--amp", action="store_true",
                   help="bf16 autocast for model math (measured slower "
                        "than --dtype bf16; kept as a recorded experiment)")
    p.add_argument("--compile", action="store_true",
                   help="torch.compile the model (dynamic shapes)")
    p.add_argument("--capture", action="store_true",
                   help="EXPERIMENTAL: hipGraph-capture fwd+bwd+opt on "
                        "statically padded shapes. Correct but measured 6x "
                        "slower on ROCm 7.0 (hipGraph per-node overhead "
                        "~130us dominates this many-small-kernel step); "
                        "kept as a recorded experiment, default off")
    p.add_argument("--graph-skew", type=float, default=0.0,
                   help="power-law skew: >0 builds a Chung-Lu graph with "
                        "lognormal(sigma=GRAPH_SKEW) expected degrees "
                        "(mean held at 2E/N) instead of uniform "
                        "Erdos-Renyi; 1.4 approximates ogbn-products' "
                        "hub-heavy histogram (max deg ~35k)")
    p.add_argument("--feature-mode", type=str, default="replicated",
                   choices=["replicated", "xgmi-shard"],
                   help="xgmi-shard: features sharded across ranks' HBM, "
                        "gathered over hip-IPC peer pointers (xGMI)")
    return p.parse_args()


def build_synthetic(args, device, rank):
    """ogbn-products-shaped random graph, built on-device.

    --graph-skew 0 (default): uniform Erdos-Renyi endpoints.
    --graph-skew s>0: Chung-Lu — both endpoints drawn with probability
    proportional to per-node lognormal(sigma=s) weights (inverse-CDF via
    searchsorted), giving the hub-heavy power-law degree histogram of
    real ogbn-products (hot-row gather contention + variable-degree
    sampler rows that the uniform graph flatters away).
    """
    import glt_amd

    glt_amd.seed_everything(args.seed + rank)
    n, e = args.nodes, args.edges
    gen_dev = device if device.type == "cuda" else torch.device("cpu")
    g = torch.Generator(device=gen_dev)
    g.manual_seed(args.seed)  # same graph on every rank
    if args.graph_skew > 0:
        w = torch.randn(n, device=gen_dev, generator=g)
        w = (w * args.graph_skew).exp()  # lognormal; mean set by normalizer
        cdf = torch.cumsum(w, 0)
        cdf /= cdf[-1].clone()
        src = torch.searchsorted(
            cdf, torch.rand(e, device=gen_dev, generator=g)).clamp_(0, n - 1)
        dst = torch.searchsorted(
            cdf, torch.rand(e, device=gen_dev, generator=g)).clamp_(0, n - 1)
    else:
        src = torch.randint(0, n, (e,), device=gen_dev, generator=g)
        dst = torch.randint(0, n, (e,), device=gen_dev, generator=g)
    # undirected: both directions
    row = torch.cat([src, dst])
    col = torch.cat([dst, src])
    # CSR build on device, sorted by (row, col) so the per-row
    # sorted-column invariant holds (the negative sampler binary-searches
    # rows; fits int64 for n < 3e9 / sqrt)
    perm = torch.argsort(row * n + col)
    row_s, col_s = row[perm], col[perm]
    counts = torch.bincount(row_s, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.long, device=gen_dev)
    torch.cumsum(counts, 0, out=indptr[1:])

    from glt_amd.data import Graph, Topology

    if args.graph_mode == "CUDA" and device.type == "cuda":
        topo = Topology((indptr, col_s), input_layout="CSR", layout="CSR",
                        auto_edge_ids=False)
    else:
        topo = Topology((indptr.cpu(), col_s.cpu()), input_layout="CSR",
                        layout="CSR", auto_edge_ids=False)
    graph = Graph(topo, mode=args.graph_mode, device=device.index)
    if args.graph_mode == "CUDA" and device.type == "cuda":
        # already on device
        graph._indptr, graph._indices = topo.indptr, topo.indices
        graph._edge_ids = graph._edge_weights = None
        graph._lazy_done = True

    feats = torch.randn(n, args.feat_dim, device=gen_dev, dtype=torch.float32)
    labels = torch.randint(0, args.classes, (n,), device=gen_dev)
    return graph, feats, labels


class _CapturedStep:
    """hipGraph capture of forward+backward+Adam over statically padded
    batch shapes (the step is launch/python-bound, not kernel-bound — see
    profiles/; one graph.replay() runs the whole ~55-kernel step).

    Static layout: region r holds hop-r nodes, sized (no-dedup cap) + 1
    reserved always-pad row; hop-r edge segment is sized frontier_cap * k,
    real edges first (targets remapped into the padded row space), then
    pad edges targeting region (r-1)'s reserved row with src = 0.  That
    keeps targets globally sorted for the fused segment kernels, keeps
    pad outputs out of every real row, and makes every shape a constant of
    (batch, fanout) so real batches always fit.
    """

    def __init__(self, model, opt, fanout, batch, feat_dim, classes,
                 device):
        self.device = device
        caps = [batch]
        for k in fanout:
            caps.append(caps[-1] * k)
        self.nsn = [c + 1 for c in caps]            # +1 reserved pad row
        self.nse = [self.nsn[i] * fanout[i] for i in range(len(fanout))]
        self.P = [0]
        for v in self.nsn:
            self.P.append(self.P[-1] + v)
        self.n_cap = self.P[-1]
        self.e_cap = sum(self.nse)
        self.batch = batch
        self.X = torch.zeros(self.n_cap, feat_dim, device=device)
        self.EI = torch.empty(2, self.e_cap, dtype=torch.long,
                              device=device)
        self.Y = torch.zeros(batch, dtype=torch.long, device=device)
        pad_tgt = torch.empty(self.e_cap, dtype=torch.long)
        e_off = 0
        for h, e in enumerate(self.nse):
            pad_tgt[e_off:e_off + e] = self.P[h + 1] - 1  # reserved row
            e_off += e
        self.pad_tgt = pad_tgt.to(device)
        self.model, self.opt = model, opt
        self._graph = None
        self._warmups = 0
        self._loss = None
        self._out = None

    def _load(self, data):
        nsn = [int(v) for v in data.num_sampled_nodes]
        nse = [int(v) for v in data.num_sampled_edges]
        pr = [0]
        for v in nsn:
            pr.append(pr[-1] + v)
        # per-row shift: compact row space -> padded row space
        shift = torch.zeros(pr[-1], dtype=torch.long, device=self.device)
        for h in range(1, len(nsn)):
            delta = self.P[h] - pr[h]
            if delta:
                shift[pr[h]:pr[h + 1]] = delta
        # node features per region
        for h in range(len(nsn)):
            self.X[self.P[h]:self.P[h] + nsn[h]].copy_(
                data.x[pr[h]:pr[h + 1]], non_blocking=True)
        # edges: pads first, then real per static hop segment
        self.EI[0].copy_(self.pad_tgt, non_blocking=True)
        self.EI[1].fill_(0)
        e_real = 0
        e_static = 0
        for h in range(len(nse)):
            seg = data.edge_index[:, e_real:e_real + nse[h]]
            self.EI[0, e_static:e_static + nse[h]].copy_(
                seg[0] + shift[seg[0]])
            self.EI[1, e_static:e_static + nse[h]].copy_(
                seg[1] + shift[seg[1]])
            e_real += nse[h]
            e_static += self.nse[h]
        self.Y.copy_(data.y[:self.batch], non_blocking=True)

    def _run(self):
        self.opt.zero_grad(set_to_none=False)
        out = self.model(self.X, self.EI, self.nsn, self.nse)[:self.batch]
        self._out = out
        loss = F.cross_entropy(out, self.Y)
        loss.backward()
        self.opt.step()
        return loss

    def step(self, data):
        self._load(data)
        if self._graph is not None:
            self._graph.replay()
            return self._loss
        self._warmups += 1
        if self._warmups <= 3:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                loss = self._run()
            torch.cuda.current_stream().wait_stream(s)
            return loss
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._loss = self._run()
        self._graph = g
        self._graph.replay()
        return self._loss


def dump_outputs(out_dir, last):
    """Write what the last timed step computed as <out_dir>/<name>.npy.

    loss and logits are what the step hands its caller; seed_nodes and
    labels identify the batch they belong to (ids are exact in float64).
    ~200 KB at the default config, so nothing needs sampling to stay
    under the 64 MB budget.

    Same arguments => same graph, features, initial weights, seed order
    and sampled neighbourhoods.  main() also switches the segment
    backward to its deterministic mode (glt_amd.ops.set_deterministic;
    the result line says "deterministic": true): its atomics then add
    grid-snapped, exactly summable terms, and the bias gradient is always
    folded in fixed order.  That is order-independent as long as no dX
    element collects more than 64x the largest |dY| of its layer; a hub
    node sampled into that many neighbourhoods of one batch (possible
    with --graph-skew) falls back to ordinary fp32 rounding for that
    element.  Under that condition two runs of one build write identical
    arrays (measured on MI355X, default graph, bf16 and fp32, after 10
    and 120 steps: max |diff| 0).  Two different builds are a
    different matter: any change in rounding is amplified by Adam step
    by step (order-dependent atomics alone gave logits max |diff| 3e-3
    after 10 steps and 3e-2 after 120), so compare builds at a small
    --steps.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    data = last["data"]
    arrays = {
        "loss": last["loss"].detach().float().reshape(1),
        "logits": last["out"].detach().float(),
        "labels": data.y[:data.batch_size].double(),
    }
    batch = getattr(data, "batch", None)
    if batch is not None:
        arrays["seed_nodes"] = batch.double()
    total = 0
    for name, t in arrays.items():
        a = t.cpu().contiguous().numpy()
        total += a.nbytes
        assert total <= 64 * 2**20, "dump exceeds 64 MB"
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    has_gpu = torch.cuda.is_available()
    if not has_gpu:
        # CPU debug mode: shrink so it finishes quickly
        args.nodes = min(args.nodes, 20_000)
        args.edges = min(args.edges, 400_000)
    # explicit --steps/--warmup are always honoured
    if args.steps is None:
        args.steps = 300 if has_gpu else 5
    if args.warmup is None:
        args.warmup = 20 if has_gpu else 2
    if args.steps < 1:
        sys.exit("--steps must be >= 1")

    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    device = torch.device("cuda", local_rank) if has_gpu \
        else torch.device("cpu")
    if has_gpu:
        torch.cuda.set_device(device)
    if world > 1:
        dist.init_process_group(
            backend="nccl" if has_gpu else "gloo",
            rank=rank, world_size=world)

    import glt_amd
    from glt_amd import Dataset, NeighborLoader
    from glt_amd.data import Feature
    from glt_amd.models import GraphSAGE
    from glt_amd.ops import set_deterministic

    # same arguments must give the same outputs run to run: take the
    # order-independent segment backward (not the library default)
    set_deterministic(True)

    fanout = [int(x) for x in args.fanout.split(",")]
    graph, feats, labels = build_synthetic(args, device, rank)

    compute_dtype = torch.bfloat16 if args.dtype == "bf16" \
        else torch.float32
    if compute_dtype != torch.float32:
        feats = feats.to(compute_dtype)
    ds = Dataset()
    ds.graph = graph
    if has_gpu and args.feature_mode == "xgmi-shard" and world > 1:
        from glt_amd.data import XgmiShardedFeature

        ds.node_features = XgmiShardedFeature(
            feats.cpu() if feats.is_cuda else feats, device=device.index)
    elif has_gpu:
        # features fully HBM-resident (288 GB): split_ratio 1.0
        f = Feature(feats.cpu() if feats.is_cuda else feats,
                    split_ratio=1.0, device=device.index, with_gpu=True)
        ds.node_features = f
    else:
        ds.node_features = Feature(feats, with_gpu=False)
    ds.node_labels = labels.to(device)

    model = GraphSAGE(args.feat_dim, args.hidden, len(fanout),
                      out_channels=args.classes).to(device)
    if args.compile:
        model = torch.compile(model, dynamic=True)
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(
            model, device_ids=[local_rank] if has_gpu else None)
    try:
        # fused Adam: one multi-tensor HIP kernel per step (less python
        # dispatch in the launch-bound regime); falls back to foreach.
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=has_gpu,
                               capturable=bool(args.capture and has_gpu))
    except (RuntimeError, ValueError):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3,
                               capturable=bool(args.capture and has_gpu))

    seeds = torch.arange(args.nodes, device=device)
    loader = NeighborLoader(ds, fanout, input_nodes=seeds,
                            batch_size=args.batch_size, shuffle=True,
                            drop_last=args.capture,
                            device=device, to_device=device,
                            prefetch=args.prefetch if has_gpu else 0)
    it = iter(loader)

    captured = None
    if args.capture and has_gpu and world == 1:
        captured = _CapturedStep(model, opt, fanout, args.batch_size,
                                 args.feat_dim, args.classes, device)

    import contextlib

    def amp_ctx():
        if args.amp and has_gpu:
            return torch.autocast("cuda", dtype=torch.bfloat16)
        return contextlib.nullcontext()

    last = {}

    def one_step():
        nonlocal it
        try:
            data = next(it)
        except StopIteration:
            it = iter(loader)
            data = next(it)
        last["data"] = data
        if captured is not None:
            last["loss"] = captured.step(data)
            last["out"] = captured._out
            return last["loss"]
        opt.zero_grad(set_to_none=True)
        with amp_ctx():
            out = model(data.x, data.edge_index, data.num_sampled_nodes,
                        data.num_sampled_edges)[:data.batch_size]
            loss = F.cross_entropy(out.float(), data.y[:data.batch_size])
        loss.backward()
        opt.step()
        # references only (no sync, no copy): --dump-outputs reads them
        # after the timed loop
        last["out"], last["loss"] = out, loss
        return loss

    # warmup
    for _ in range(args.warmup):
        one_step()
    if has_gpu:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    if has_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], device=device if has_gpu else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    loader.shutdown()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    batches_per_sec = args.steps / elapsed * world
    ms_per_step = elapsed / args.steps * 1000.0
    # ogbn-products train split: 196,615 seeds -> epoch equivalent
    epoch_batches = (196_615 + args.batch_size - 1) // args.batch_size
    if rank == 0:
        print(json.dumps({
            "metric": "GraphSAGE ogbn-products(synthetic) train batches/sec",
            "value": round(batches_per_sec, 3),
            "unit": "batches/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if (args.amp or args.dtype == "bf16")
                     else "fp32",
            "data": "synthetic",
            "deterministic": True,
            "config": {
                "model": "GraphSAGE(3x256)",
                "global_batch": args.batch_size * world,
                "fanout": fanout,
                "nodes": args.nodes,
                "edges_undirected": args.edges,
                "feat_dim": args.feat_dim,
                "classes": args.classes,
                "graph_mode": args.graph_mode,
                "graph_skew": args.graph_skew,
                "parallelism": f"dp{world}",
                "feature_mode": args.feature_mode,
                "epoch_time_s_equiv": round(
                    epoch_batches / (batches_per_sec / world), 3),
            },
        }))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

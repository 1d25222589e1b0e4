"""NeighborSampler — the local multi-hop sampling engine.

Capability parity: reference python/sampler/neighbor_sampler.py (homo &
hetero multi-hop :169-317, sample_from_edges with binary/triplet negatives
:319-446, subgraph :474-498, sample_prob :500-627).  Fresh implementation:
one code path for CPU and GPU (native ops auto-dispatch on tensor device),
hetero induction orchestrated in python over per-type native inducers,
row expansion via torch.repeat_interleave instead of bespoke kernels.
"""
import threading
from typing import Dict, List, Optional, Union

import torch

from ..data import Graph
from ..typing import EdgeType, NodeType, reverse_edge_type
from ..utils.tracing import trace_region
from .base import (BaseSampler, EdgeSamplerInput, HeteroSamplerOutput,
                   NegativeSampling, NeighborOutput, NodeSamplerInput,
                   SamplerOutput)


def _relabel(uniq: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """Positions of `ids` within insertion-ordered unique list `uniq`."""
    sorted_uniq, perm = torch.sort(uniq)
    pos = torch.searchsorted(sorted_uniq, ids)
    return perm[pos]


class _PyHeteroInducer:
    """Device-agnostic hetero inducer over per-type native inducers."""

    def __init__(self, make_inducer):
        self._make = make_inducer
        self._inducers: Dict[NodeType, object] = {}
        self._uniq: Dict[NodeType, torch.Tensor] = {}

    def _get(self, ntype):
        if ntype not in self._inducers:
            self._inducers[ntype] = self._make()
        return self._inducers[ntype]

    def init_node(self, seed_dict: Dict[NodeType, torch.Tensor]):
        # keep per-type inducers across batches (capacity retained);
        # init_node on a native inducer resets its table
        self._uniq = {}
        out = {}
        for ntype, seeds in seed_dict.items():
            ind = self._get(ntype)
            uniq = ind.init_node(seeds)
            self._uniq[ntype] = uniq
            out[ntype] = uniq
        return out

    def insert(self, ntype, ids: torch.Tensor) -> torch.Tensor:
        ind = self._get(ntype)
        if ntype not in self._uniq:
            fresh = ind.init_node(ids)
        elif hasattr(ind, "insert"):
            fresh = ind.insert(ids)
        else:  # CPUInducer path: emulate insert via induce_next with dummy src
            fresh, _, _ = ind.induce_next(
                torch.empty(0, dtype=torch.long), ids,
                torch.empty(0, dtype=torch.long))
        self._uniq[ntype] = (torch.cat([self._uniq[ntype], fresh])
                             if ntype in self._uniq else fresh)
        return fresh

    def insert_staged(self, batch):
        """Insert [(ntype, ids), ...] of ONE hop with a single host sync
        (per-type index bias keeps the fresh-node order identical to
        sequential inserts).  Falls back to sequential insert for CPU
        inducers and first-touch types."""
        if not batch:
            return []
        stageable = []
        for ntype, ids in batch:
            ind = self._get(ntype)
            stageable.append(ntype in self._uniq
                             and hasattr(ind, "insert_begin")
                             and ids.is_cuda)
        if not all(stageable):
            return [self.insert(nt, ids) for nt, ids in batch]
        totals: Dict[NodeType, int] = {}
        for ntype, ids in batch:
            totals[ntype] = totals.get(ntype, 0) + ids.numel()
        for ntype, tot in totals.items():
            self._inducers[ntype].reserve_incoming(tot)
        base: Dict[NodeType, int] = {}
        pend = []
        for ntype, ids in batch:
            b = base.get(ntype, 0)
            flags, ranks = self._inducers[ntype].insert_begin(ids, b)
            base[ntype] = b + ids.numel()
            pend.append((ntype, ids, flags, ranks))
        dev = pend[0][1].device
        zero = torch.zeros(1, dtype=torch.long, device=dev)
        n_new = torch.cat(
            [(p[3][-1:] if p[3].numel() else zero) for p in pend]
        ).cpu()  # the hop's single insert sync
        fresh_list = []
        for (ntype, ids, flags, ranks), nn in zip(pend, n_new.tolist()):
            fresh = self._inducers[ntype].insert_commit(ids, flags, ranks,
                                                       int(nn))
            self._uniq[ntype] = torch.cat([self._uniq[ntype], fresh])
            fresh_list.append(fresh)
        return fresh_list

    def lookup(self, ntype, ids: torch.Tensor) -> torch.Tensor:
        ind = self._inducers[ntype]
        if hasattr(ind, "lookup"):
            return ind.lookup(ids)
        return _relabel(self._uniq[ntype], ids)

    def nodes(self, ntype):
        return self._uniq.get(ntype)


class NeighborSampler(BaseSampler):
    """Multi-hop neighbor sampler over a Graph (homo) or Dict[EdgeType,
    Graph] (hetero)."""

    def __init__(self, graph: Union[Graph, Dict[EdgeType, Graph]],
                 num_neighbors: Optional[List[int]] = None,
                 device: Optional[torch.device] = None,
                 with_edge: bool = False, with_neg: bool = False,
                 with_weight: bool = False, edge_dir: str = "out",
                 seed: Optional[int] = None,
                 weight_replace: bool = True,
                 time_attr: Optional[str] = None,
                 node_time: Optional[torch.Tensor] = None,
                 temporal_strategy: str = "uniform"):
        """time_attr: None, 'node' or 'edge' — temporal sampling: a seed
        observed at time t only sees neighbours with time <= t, the time
        being node_time[neighbour] ('node') or the graph's edge_times
        ('edge').  temporal_strategy: 'uniform' or 'last' (most recent
        first).  Temporal sampling is disjoint: every seed slot grows its
        own tree (see _temporal_sample_from_nodes)."""
        from .. import _C

        self._C = _C
        self.graph = graph
        self.num_neighbors = num_neighbors
        self.with_edge = with_edge
        self.with_neg = with_neg
        self.with_weight = with_weight
        # weighted draws: with replacement (reference semantics) or
        # Efraimidis-Spirakis without replacement (GPU+CPU kernels)
        self.weight_replace = weight_replace
        self.edge_dir = edge_dir
        self.is_hetero = isinstance(graph, dict)
        self._lock = threading.Lock()
        self._inducer_pool = []
        self._hetero_pool = []
        if seed is not None:
            _C.manual_seed(seed)
        g0 = next(iter(graph.values())) if self.is_hetero else graph
        # Sampling always runs where the graph's CSR lives (device tensors
        # for CUDA/ZERO_COPY modes, host for CPU mode); `device` only sets
        # where outputs are reported.
        self._sample_device = g0.indptr.device
        self.device = torch.device(device) if device is not None \
            else self._sample_device
        self._cpu_mode = self._sample_device.type == "cpu"
        # Deferred-sync fast path (GPU homo uniform sampling): the whole
        # multi-hop batch runs with device-resident counts and ONE host
        # sync at the end (see csrc/hip/hip_deferred.hip).  Capacity
        # buffers are worst-case (batch x prod(fanout)); gate on a sane
        # edge cap so exotic fan-outs fall back to the classic path.
        self._deferred_pool = []
        nn = self.num_neighbors
        self.use_deferred = (
            not self._cpu_mode and not self.is_hetero
            and isinstance(nn, (list, tuple)) and len(nn) > 0
            and all(isinstance(k, int) and k > 0 for k in nn)
            and not (self.with_weight and g0.edge_weights is not None))
        self._deferred_with_eid = (self.with_edge
                                   and g0.edge_ids is not None
                                   if not self.is_hetero else False)
        self.time_attr = time_attr
        self.temporal_strategy = temporal_strategy
        self.node_time = None
        if time_attr is not None:
            self._init_temporal(g0, node_time)

    def _init_temporal(self, g0, node_time):
        if self.time_attr not in ("node", "edge"):
            raise ValueError(
                f"time_attr must be None, 'node' or 'edge', got "
                f"{self.time_attr!r}")
        if self.temporal_strategy not in ("uniform", "last"):
            raise ValueError(
                f"temporal_strategy must be 'uniform' or 'last', got "
                f"{self.temporal_strategy!r}")
        if self.is_hetero:
            raise NotImplementedError(
                "time_attr: temporal sampling on heterogeneous graphs is "
                "not implemented")
        if self.with_weight:
            raise NotImplementedError(
                "time_attr: weighted temporal draws are not implemented "
                "(with_weight=True)")
        if self.time_attr == "edge":
            if g0.edge_times is None:
                raise ValueError(
                    "time_attr='edge' needs a graph built with edge_times")
        else:
            if node_time is None:
                raise ValueError("time_attr='node' needs node_time")
            node_time = torch.as_tensor(node_time)
            if node_time.dim() != 1 or node_time.is_floating_point():
                raise ValueError("node_time must be a 1-D integer tensor")
            if node_time.numel() < g0.num_nodes:
                raise ValueError("node_time must cover every node")
            self.node_time = node_time.long().contiguous().to(
                self._sample_device)
        self.use_deferred = False  # the deferred kernels know no times
        # Composite-key modulus of the disjoint bookkeeping: greater than
        # every row and every id in indices.
        idx = g0.topo.indices
        self._temporal_mod = max(
            int(g0.num_nodes),
            int(idx.max()) + 1 if idx.numel() else 0,
            self.node_time.numel() if self.node_time is not None else 0, 1)

    # ------------------------------------------------------------------
    def _make_inducer(self):
        if self._cpu_mode:
            return self._C.CPUInducer(1024)
        return self._C.DeviceInducer(65536)

    def _acquire_inducer(self):
        """Reuse inducers across batches: their hash-table capacity is
        retained, so steady-state batches skip allocation and the
        growth-rebuild inserts."""
        with self._lock:
            if self._inducer_pool:
                return self._inducer_pool.pop()
        return self._make_inducer()

    def _release_inducer(self, ind):
        with self._lock:
            if len(self._inducer_pool) < 8:
                self._inducer_pool.append(ind)

    def _acquire_hetero_inducer(self):
        with self._lock:
            if self._hetero_pool:
                return self._hetero_pool.pop()
        return _PyHeteroInducer(self._make_inducer)

    def _release_hetero_inducer(self, ind):
        with self._lock:
            if len(self._hetero_pool) < 8:
                self._hetero_pool.append(ind)

    def _seeds_to_device(self, seeds: torch.Tensor) -> torch.Tensor:
        return seeds.long().to(self._sample_device, non_blocking=True)

    def _sample_hop_batched(self, reqs):
        """One hop over several edge types with a SINGLE host sync.

        The classic path synced once per (hop, etype) inside
        sample_neighbors (the edge-total read); those GIL-held device
        waits in the producer thread throttled the launch-bound hetero
        consumer (measured: RGAT model-only 250 b/s vs pipelined
        ~150-210, ROUND2_NOTES).  Stage 1 launches every etype's
        count+cumsum, ONE .cpu() reads all totals, stage 2 gathers.
        Draw order matches the classic path (fresh_seed per etype in
        iteration order), so outputs are bit-identical.
        """
        if not reqs:
            return []
        gpu = all(self.graph[et].indptr.is_cuda for et, _, _ in reqs)
        if not gpu:
            return [(et, srcs, self.sample_one_hop(srcs, k, etype=et))
                    for et, srcs, k in reqs]
        staged = []
        for etype, srcs, k in reqs:
            g = self.graph[etype]
            srcs_d = srcs.to(g.indptr.device, non_blocking=True)
            counts, offsets = self._C.sample_neighbors_offsets(
                g.indptr, srcs_d, k)
            staged.append((etype, srcs, srcs_d, k, g, counts, offsets))
        totals = torch.stack(
            [st[6][-1] for st in staged]).cpu()  # the hop's ONE sync
        results = []
        for (etype, srcs, srcs_d, k, g, counts, offsets), tot in zip(
                staged, totals.tolist()):
            weighted = self.with_weight and g.edge_weights is not None
            nbrs, eids = self._C.sample_neighbors_gather(
                g.indptr, g.indices, srcs_d, k, offsets, int(tot),
                edge_ids=g.edge_ids if self.with_edge else None,
                edge_weights=g.edge_weights if weighted else None,
                with_edge=self.with_edge, weighted=weighted,
                replace=getattr(self, "weight_replace", True))
            results.append((etype, srcs,
                            NeighborOutput(nbrs, counts, eids)))
        return results

    def sample_one_hop(self, srcs: torch.Tensor, k: int,
                       etype: Optional[EdgeType] = None) -> NeighborOutput:
        """Uniform (or weighted) one-hop sample from srcs."""
        g = self.graph[etype] if etype is not None else self.graph
        # sampling runs where the CSR lives, whatever device srcs arrive on
        srcs = srcs.to(g.indptr.device, non_blocking=True)
        weighted = self.with_weight and g.edge_weights is not None
        nbrs, num, eids = self._C.sample_neighbors(
            g.indptr, g.indices, srcs, k,
            edge_ids=g.edge_ids if self.with_edge else None,
            edge_weights=g.edge_weights if weighted else None,
            with_edge=self.with_edge, weighted=weighted,
            replace=getattr(self, "weight_replace", True))
        return NeighborOutput(nbrs, num, eids)

    # -- homo ----------------------------------------------------------
    def sample_from_nodes(self, inputs: NodeSamplerInput,
                          **kwargs) -> Union[SamplerOutput,
                                             HeteroSamplerOutput]:
        if self.is_hetero:
            return self._hetero_sample_from_nodes(inputs)
        seeds = self._seeds_to_device(inputs.node)
        if self.time_attr is not None:
            with trace_region("sample_from_nodes_temporal"):
                return self._temporal_sample_from_nodes(
                    seeds, self._seed_times(seeds, inputs.time),
                    metadata={"input_type": None})
        with trace_region("sample_from_nodes"):
            return self._sample_from_nodes(seeds,
                                           metadata={"input_type": None})

    # -- temporal (disjoint) ---------------------------------------------
    def _seed_times(self, seeds: torch.Tensor,
                    time: Optional[torch.Tensor]) -> torch.Tensor:
        if time is None:
            if self.time_attr != "node":
                raise ValueError(
                    "time_attr='edge' needs seed times (input_time= / "
                    "NodeSamplerInput.time)")
            return self.node_time[seeds]  # PyG: the seeds' own time
        time = torch.as_tensor(time)
        if time.numel() != seeds.numel():
            raise ValueError("seed times must have one entry per seed")
        return time.long().to(self._sample_device,
                              non_blocking=True).contiguous()

    def sample_one_hop_temporal(self, srcs: torch.Tensor,
                                src_time: torch.Tensor,
                                k: int) -> NeighborOutput:
        """One-hop sample from srcs, slot i seeing only edges with
        time <= src_time[i]."""
        g = self.graph
        by_edge = self.time_attr == "edge"
        nbrs, num, eids = self._C.sample_neighbors_temporal(
            g.indptr, g.indices, srcs.contiguous(), src_time.contiguous(),
            k, edge_ids=g.edge_ids if self.with_edge else None,
            edge_time=g.edge_times if by_edge else None,
            node_time=None if by_edge else self.node_time,
            with_edge=self.with_edge,
            last=self.temporal_strategy == "last")
        return NeighborOutput(nbrs, num, eids)

    def _temporal_sample_from_nodes(self, seeds: torch.Tensor,
                                    seed_time: torch.Tensor,
                                    metadata=None) -> SamplerOutput:
        """Disjoint multi-hop sampling: every seed slot grows its own tree
        and a node's time bound at every hop is the seed time of its slot.
        Nodes are deduplicated per (slot, node id) by feeding the inducers
        composite keys slot * M + node id; two equal seeds stay two slots.
        """
        dev = self._sample_device
        bs = seeds.numel()
        M = self._temporal_mod
        assert bs * M < 2 ** 63, "batch_size * M overflows the inducer keys"
        slots = torch.arange(bs, dtype=torch.long, device=dev)
        inducer = self._acquire_inducer()
        src_keys = inducer.init_node(slots * M + seeds)  # all distinct
        src_nodes, src_slots = seeds, slots
        out_nodes, out_slots = [seeds], [slots]
        num_nodes, num_edges = [bs], []
        rows, cols, eids = [], [], []
        for k in (self.num_neighbors or []):
            out = self.sample_one_hop_temporal(src_nodes,
                                               seed_time[src_slots], k)
            total = out.nbr.numel()
            slot_of_nbr = torch.repeat_interleave(src_slots, out.nbr_num,
                                                  output_size=total)
            new_keys, r, c = inducer.induce_next(
                src_keys, slot_of_nbr * M + out.nbr, out.nbr_num)
            src_keys = new_keys
            src_nodes = new_keys % M
            src_slots = torch.div(new_keys, M, rounding_mode="floor")
            out_nodes.append(src_nodes)
            out_slots.append(src_slots)
            num_nodes.append(src_nodes.numel())
            num_edges.append(r.numel())
            rows.append(r)
            cols.append(c)
            if out.edge is not None:
                eids.append(out.edge)
        self._release_inducer(inducer)
        empty = torch.empty(0, dtype=torch.long, device=dev)
        md = dict(metadata or {})
        md["seed_index"] = torch.cat(out_slots)
        md["seed_time"] = seed_time
        return SamplerOutput(
            node=torch.cat(out_nodes),
            row=torch.cat(rows) if rows else empty,
            col=torch.cat(cols) if cols else empty,
            edge=torch.cat(eids) if eids else None, batch=seeds,
            num_sampled_nodes=num_nodes, num_sampled_edges=num_edges,
            device=self.device, metadata=md)

    # -- deferred-sync fast path ---------------------------------------
    def _acquire_deferred(self, bs: int):
        with self._lock:
            for i, (cap, ds) in enumerate(self._deferred_pool):
                if cap >= bs:
                    return self._deferred_pool.pop(i)
        cap = max(1024, 1 << (bs - 1).bit_length())
        ds = self._C.DeferredSampler(
            list(self.num_neighbors), cap,
            self._sample_device.index or 0, self._deferred_with_eid)
        return (cap, ds)

    def _release_deferred(self, entry):
        with self._lock:
            if len(self._deferred_pool) < 8:
                self._deferred_pool.append(entry)

    def _edge_cap(self, bs: int) -> int:
        total, cap = 0, bs
        for k in self.num_neighbors:
            cap *= k
            total += cap
        return total

    def _sample_from_nodes_deferred(self, seeds: torch.Tensor,
                                    metadata=None) -> SamplerOutput:
        g = self.graph
        entry = self._acquire_deferred(seeds.numel())
        node_parts, rows, cols, eids, stats = entry[1].run(
            g.indptr, g.indices,
            g.edge_ids if self._deferred_with_eid else None, seeds)
        s = stats.cpu().tolist()  # the batch's single host sync
        L = len(self.num_neighbors)
        n_new, e_tot = s[:L + 1], s[L + 1:]
        node = torch.cat([node_parts[i][:n_new[i]] for i in range(L + 1)])
        row = torch.cat([rows[h][:e_tot[h]] for h in range(L)])
        col = torch.cat([cols[h][:e_tot[h]] for h in range(L)])
        edge = (torch.cat([eids[h][:e_tot[h]] for h in range(L)])
                if eids else None)
        self._release_deferred(entry)
        return SamplerOutput(
            node=node, row=row, col=col, edge=edge, batch=node[:n_new[0]],
            num_sampled_nodes=n_new, num_sampled_edges=e_tot,
            device=self.device, metadata=metadata)

    def _sample_from_nodes(self, seeds: torch.Tensor,
                           metadata=None) -> SamplerOutput:
        if self.use_deferred and self._edge_cap(seeds.numel()) <= (1 << 25):
            return self._sample_from_nodes_deferred(seeds, metadata)
        inducer = self._acquire_inducer()
        uniq_seeds = inducer.init_node(seeds)
        out_nodes = [uniq_seeds]
        num_nodes = [uniq_seeds.numel()]
        num_edges = []
        rows, cols, eids = [], [], []
        srcs = uniq_seeds
        for k in (self.num_neighbors or []):
            out = self.sample_one_hop(srcs, k)
            nodes, r, c = inducer.induce_next(srcs, out.nbr, out.nbr_num)
            out_nodes.append(nodes)
            num_nodes.append(nodes.numel())
            num_edges.append(r.numel())
            rows.append(r)
            cols.append(c)
            if out.edge is not None:
                eids.append(out.edge)
            srcs = nodes
        node = torch.cat(out_nodes)
        row = torch.cat(rows) if rows else torch.empty(
            0, dtype=torch.long, device=self.device)
        col = torch.cat(cols) if cols else torch.empty(
            0, dtype=torch.long, device=self.device)
        edge = torch.cat(eids) if eids else None
        self._release_inducer(inducer)
        return SamplerOutput(
            node=node, row=row, col=col, edge=edge, batch=uniq_seeds,
            num_sampled_nodes=num_nodes, num_sampled_edges=num_edges,
            device=self.device, metadata=metadata)

    # -- hetero ---------------------------------------------------------
    def _etype_fanout(self, etype: EdgeType, hop: int) -> int:
        nn = self.num_neighbors
        if isinstance(nn, dict):
            fan = nn.get(etype)
            if fan is None:
                return 0
            return fan[hop] if hop < len(fan) else 0
        return nn[hop] if nn and hop < len(nn) else 0

    def _num_hops(self) -> int:
        nn = self.num_neighbors
        if isinstance(nn, dict):
            return max(len(v) for v in nn.values())
        return len(nn or [])

    def _hetero_sample_from_nodes(
            self, inputs: NodeSamplerInput) -> HeteroSamplerOutput:
        input_type = inputs.input_type
        assert input_type is not None, "hetero sampling needs input_type"
        seeds = self._seeds_to_device(inputs.node)
        return self._hetero_multihop(
            {input_type: seeds},
            metadata={"input_type": input_type, "bs": seeds.numel()})

    def _hetero_multihop(self, seed_dict: Dict[NodeType, torch.Tensor],
                         metadata=None) -> HeteroSamplerOutput:
        inducer = self._acquire_hetero_inducer()
        frontier = inducer.init_node(seed_dict)
        out_nodes: Dict[NodeType, List[torch.Tensor]] = {
            t: [v] for t, v in frontier.items()}
        num_nodes = {t: [v.numel()] for t, v in frontier.items()}
        rows: Dict[EdgeType, List[torch.Tensor]] = {}
        cols: Dict[EdgeType, List[torch.Tensor]] = {}
        eids: Dict[EdgeType, List[torch.Tensor]] = {}
        num_edges: Dict[EdgeType, List[int]] = {}

        for hop in range(self._num_hops()):
            next_frontier: Dict[NodeType, List[torch.Tensor]] = {}
            reqs = []
            for etype, g in self.graph.items():
                # In 'out' mode an etype (src, rel, dst) is sampled from its
                # src-type frontier; in 'in' mode graphs are CSC keyed the
                # same but we walk from dst.
                walk_from = etype[0] if self.edge_dir == "out" else etype[2]
                srcs = frontier.get(walk_from)
                if srcs is None or srcs.numel() == 0:
                    continue
                k = self._etype_fanout(etype, hop)
                if k == 0:
                    continue
                reqs.append((etype, srcs, k))
            hop_results = self._sample_hop_batched(reqs)
            # Phase 1: insert all new nodes (deterministic etype order;
            # staged — one host sync for the whole hop's inserts).
            intos = [etype[2] if self.edge_dir == "out" else etype[0]
                     for etype, _, _ in hop_results]
            fresh_all = inducer.insert_staged(
                [(into, out.nbr)
                 for into, (_, _, out) in zip(intos, hop_results)])
            for into, fresh in zip(intos, fresh_all):
                out_nodes.setdefault(into, []).append(fresh)
                num_nodes.setdefault(into, []).append(fresh.numel())
                next_frontier.setdefault(into, []).append(fresh)
            # Phase 2: relabel edges.  For edge_dir='in' the walk goes
            # dst->src over CSC, so results are stored under the reversed
            # edge type (reference neighbor_sampler.py:261-269).
            for etype, srcs, out in hop_results:
                src_t = etype[0] if self.edge_dir == "out" else etype[2]
                dst_t = etype[2] if self.edge_dir == "out" else etype[0]
                key = (etype if self.edge_dir == "out"
                       else reverse_edge_type(etype))
                src_local = inducer.lookup(src_t, srcs)
                r = torch.repeat_interleave(src_local, out.nbr_num)
                c = inducer.lookup(dst_t, out.nbr)
                rows.setdefault(key, []).append(r)
                cols.setdefault(key, []).append(c)
                num_edges.setdefault(key, []).append(r.numel())
                if out.edge is not None:
                    eids.setdefault(key, []).append(out.edge)
            frontier = {t: torch.cat(v) for t, v in next_frontier.items()
                        if v}
        node = {t: torch.cat(v) for t, v in out_nodes.items()}
        row = {et: torch.cat(v) for et, v in rows.items()}
        col = {et: torch.cat(v) for et, v in cols.items()}
        edge = {et: torch.cat(v) for et, v in eids.items()} if eids else None
        batch = {t: self._uniq_of(seed_dict, inducer, t)
                 for t in seed_dict.keys()}
        self._release_hetero_inducer(inducer)
        return HeteroSamplerOutput(
            node=node, row=row, col=col, edge=edge, batch=batch,
            num_sampled_nodes=num_nodes, num_sampled_edges=num_edges,
            edge_types=list(self.graph.keys()),
            input_type=(metadata or {}).get("input_type"),
            device=self.device, metadata=metadata)

    @staticmethod
    def _uniq_of(seed_dict, inducer, t):
        n = inducer.nodes(t)
        # seeds of type t are the first len(unique seeds) entries
        return n[: torch.unique(seed_dict[t]).numel()] if n is not None \
            else seed_dict[t]

    # -- link sampling ---------------------------------------------------
    def sample_from_edges(self, inputs: EdgeSamplerInput,
                          **kwargs) -> Union[SamplerOutput,
                                             HeteroSamplerOutput]:
        if self.time_attr is not None:
            raise NotImplementedError(
                "time_attr: temporal link sampling (sample_from_edges) is "
                "not implemented")
        neg = inputs.neg_sampling
        if self.is_hetero:
            return self._hetero_sample_from_edges(inputs)
        row = self._seeds_to_device(inputs.row)
        col = self._seeds_to_device(inputs.col)
        num_pos = row.numel()
        g = self.graph
        if neg is not None and neg.is_binary():
            num_neg = int(num_pos * neg.amount)
            neg_edges = self._C.sample_negative(
                g.indptr, g.indices, g.num_nodes, num_neg, 5, True)
            seeds = torch.cat([row, col, neg_edges[0], neg_edges[1]])
            out = self._sample_from_nodes(seeds)
            local = _relabel_through(self, out, seeds)
            n_neg = neg_edges.size(1)
            eli = torch.stack([
                torch.cat([local[:num_pos], local[2 * num_pos:
                                                  2 * num_pos + n_neg]]),
                torch.cat([local[num_pos:2 * num_pos],
                           local[2 * num_pos + n_neg:]]),
            ])
            label = torch.cat([
                inputs.label.to(self.device) if inputs.label is not None
                else torch.ones(num_pos, device=self.device),
                torch.zeros(n_neg, device=self.device),
            ])
            out.metadata = {"edge_label_index": eli, "edge_label": label,
                            "input_type": None}
            return out
        if neg is not None and neg.is_triplet():
            amount = int(neg.amount)
            neg_dst = self._C.sample_negative(
                g.indptr, g.indices, g.num_nodes, num_pos * amount, 5,
                True)[1]
            seeds = torch.cat([row, col, neg_dst])
            out = self._sample_from_nodes(seeds)
            local = _relabel_through(self, out, seeds)
            out.metadata = {
                "src_index": local[:num_pos],
                "dst_pos_index": local[num_pos:2 * num_pos],
                "dst_neg_index":
                    local[2 * num_pos:].view(num_pos, amount)
                    if local.numel() >= 2 * num_pos else local[2 * num_pos:],
                "input_type": None,
            }
            return out
        seeds = torch.cat([row, col])
        out = self._sample_from_nodes(seeds)
        local = _relabel_through(self, out, seeds)
        eli = torch.stack([local[:num_pos], local[num_pos:]])
        label = (inputs.label.to(self.device)
                 if inputs.label is not None else None)
        out.metadata = {"edge_label_index": eli, "edge_label": label,
                        "input_type": None}
        return out

    def _hetero_sample_from_edges(
            self, inputs: EdgeSamplerInput) -> HeteroSamplerOutput:
        etype = inputs.input_type
        assert etype is not None
        src_t, _, dst_t = etype
        row = self._seeds_to_device(inputs.row)
        col = self._seeds_to_device(inputs.col)
        num_pos = row.numel()
        neg = inputs.neg_sampling
        neg_dst = None
        if neg is not None:
            g = self.graph[etype]
            amount = (int(num_pos * neg.amount) if neg.is_binary()
                      else num_pos * int(neg.amount))
            neg_pair = self._C.sample_negative(
                g.indptr, g.indices, g.num_nodes, amount, 5, True)
            neg_dst = neg_pair[1]
        if src_t == dst_t:
            seeds = {src_t: torch.cat([row, col] +
                                      ([neg_dst] if neg_dst is not None
                                       else []))}
        else:
            dst_seeds = torch.cat([col] + ([neg_dst]
                                           if neg_dst is not None else []))
            seeds = {src_t: row, dst_t: dst_seeds}
        out = self._hetero_multihop(seeds, metadata={"input_type": etype})
        src_local = _relabel(out.node[src_t], row)
        dst_local = _relabel(out.node[dst_t], col)
        if neg is not None and neg.is_triplet():
            out.metadata.update({
                "src_index": src_local,
                "dst_pos_index": dst_local,
                "dst_neg_index": _relabel(out.node[dst_t],
                                          neg_dst).view(num_pos, -1),
            })
        else:
            if neg_dst is not None:
                neg_src = row.repeat(
                    (neg_dst.numel() + num_pos - 1) // num_pos)[
                        : neg_dst.numel()]
                eli = torch.stack([
                    torch.cat([src_local,
                               _relabel(out.node[src_t], neg_src)]),
                    torch.cat([dst_local,
                               _relabel(out.node[dst_t], neg_dst)]),
                ])
                label = torch.cat([
                    torch.ones(num_pos, device=self.device),
                    torch.zeros(neg_dst.numel(), device=self.device)])
            else:
                eli = torch.stack([src_local, dst_local])
                label = (inputs.label.to(self.device)
                         if inputs.label is not None else None)
            out.metadata.update({"edge_label_index": eli,
                                 "edge_label": label})
        return out

    # -- subgraph ---------------------------------------------------------
    def subgraph(self, inputs: NodeSamplerInput) -> SamplerOutput:
        """Induce the full edge set among the (optionally multi-hop
        expanded) seed set (SamplingType.SUBGRAPH; e.g. SEAL)."""
        seeds = self._seeds_to_device(inputs.node)
        g = self.graph
        nodes = seeds
        for k in (self.num_neighbors or []):
            out = self.sample_one_hop(nodes, k)
            nodes = torch.cat([nodes, out.nbr])
        uniq, rows, cols, eids = self._C.node_subgraph(
            g.indptr, g.indices, nodes, edge_ids=g.edge_ids,
            with_edge=self.with_edge)
        return SamplerOutput(
            node=uniq, row=rows, col=cols, edge=eids, device=self.device,
            metadata={"batch_size": seeds.numel(), "input_type": None})

    # -- random walk -------------------------------------------------------
    def random_walk(self, seeds: torch.Tensor, walk_len: int) -> torch.Tensor:
        g = self.graph
        return self._C.random_walk(g.indptr, g.indices,
                                   self._seeds_to_device(seeds), walk_len)

    # -- importance probability (trim) --------------------------------------
    def sample_prob(self, seeds: torch.Tensor,
                    num_nodes: Optional[int] = None) -> torch.Tensor:
        """Per-node inclusion probability after the configured multi-hop
        sampling from `seeds` (reference sample_prob,
        neighbor_sampler.py:500-627)."""
        g = self.graph
        n = num_nodes or g.num_nodes
        seeds = self._seeds_to_device(seeds)
        prob = torch.zeros(n, dtype=torch.float32, device=self.device)
        prob[seeds] = 1.0
        frontier = seeds
        for k in (self.num_neighbors or []):
            prob = self._C.cal_nbr_prob(g.indptr, g.indices, prob, frontier,
                                        k)
            frontier = torch.nonzero(prob > 0).flatten()
        return prob


def _relabel_through(sampler: NeighborSampler, out: SamplerOutput,
                     seeds: torch.Tensor) -> torch.Tensor:
    """Local positions of `seeds` in out.node (insertion-ordered)."""
    n_seed_nodes = out.num_sampled_nodes[0] if out.num_sampled_nodes else \
        out.node.numel()
    return _relabel(out.node[:n_seed_nodes], seeds)

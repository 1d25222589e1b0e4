#!/usr/bin/env python3
"""Single-kernel microbench harness — the target for rocprofv3 --pmc runs.

rocprofv3 PMC collection serializes every dispatch, so counters must be
collected over a few dispatches of ONE kernel, not the full training
pipeline.  This harness builds flagship-shaped inputs
for one chosen op and runs exactly --iters dispatches of it.

    gpurun -- 'cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT && \
      rocprofv3 --pmc SQ_INSTS_MFMA,FETCH_SIZE,WRITE_SIZE --kernel-trace \
      --stats -d gpurun_out/pmc -- \
      python tools/kernel_microbench.py --op seg_mean_cat --iters 20'
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def build_flagship_shapes(op, device, bf16=False):
    """Layer-1-of-flagship shapes: ~590k rows, 890k edges, F=100/256."""
    torch.manual_seed(0)
    n_src, n_tgt, E, F = 590_000, 130_000, 890_000, 256
    if op in ("seg_wsum", "seg_wsum_bf16", "gcn_conv",
              "gcn_conv_composite", "seg_max", "seg_max_cat",
              "sage_conv_max", "sage_conv_max_composite") or \
            (bf16 and op in ("seg_mean", "seg_mean_cat")):
        # F=256 fp32, or the bf16 feature-store shape F=100
        if op == "seg_wsum_bf16" or bf16:
            x = torch.randn(n_src, 100, device=device).to(torch.bfloat16)
        else:
            x = torch.randn(n_src, F, device=device)
        tgt = torch.sort(torch.randint(0, n_tgt, (E,), device=device))[0]
        src = torch.randint(0, n_src, (E,), device=device)
        return (x, tgt, src, n_tgt)
    if op in ("seg_mean", "seg_mean_cat"):
        x = torch.randn(n_src, F, device=device)
        tgt = torch.sort(torch.randint(0, n_tgt, (E,), device=device))[0]
        src = torch.randint(0, n_src, (E,), device=device)
        return (x, tgt, src, n_tgt)
    if op in ("gat_fused", "gat_fused_bwd"):
        H, C = 4, 64
        h = torch.randn(n_src, H, C, device=device)
        att = torch.randn(H, C, device=device)
        tgt = torch.sort(torch.randint(0, n_tgt, (E,), device=device))[0]
        src = torch.randint(0, n_src, (E,), device=device)
        return (h, att, tgt, src, n_tgt)
    if op == "mfma_gemm":
        A = torch.randn(130_000, 512, device=device)
        B = torch.randn(128, 512, device=device)
        return (A, B)
    if op == "gemm_bt_bf16":
        A = torch.randn(164_000, 200, device=device).to(torch.bfloat16)
        W = torch.randn(256, 200, device=device).to(torch.bfloat16)
        b = torch.randn(256, device=device)
        return (A, W, b)
    if op == "gemm_kt_bf16":
        A = torch.randn(164_000, 256, device=device).to(torch.bfloat16)
        B = torch.randn(164_000, 200, device=device).to(torch.bfloat16)
        return (A, B)
    if op == "seg_mean_cat_bf16":
        n_src, n_tgt, E, F = 590_000, 130_000, 890_000, 100
        x = torch.randn(n_src, F, device=device).to(torch.bfloat16)
        tgt = torch.sort(torch.randint(0, n_tgt, (E,), device=device))[0]
        src = torch.randint(0, n_src, (E,), device=device)
        return (x, tgt, src, n_tgt)
    if op == "gather":
        feats = torch.randn(2_449_029, 100, device=device)
        rows = torch.randint(0, feats.size(0), (736_000,), device=device)
        return (feats, rows)
    if op == "sample":
        n, deg = 2_449_029, 25
        indptr = torch.arange(0, (n + 1) * deg, deg, device=device)
        indices = torch.randint(0, n, (n * deg,), device=device)
        seeds = torch.randint(0, n, (131_072,), device=device)
        return (indptr, indices, seeds)
    if op in ("sample_weighted", "sample_weighted_nr"):
        n, deg = 500_000, 50
        indptr = torch.arange(0, (n + 1) * deg, deg, device=device)
        indices = torch.randint(0, n, (n * deg,), device=device)
        w = torch.rand(n * deg, device=device)
        seeds = torch.randint(0, n, (131_072,), device=device)
        return (indptr, indices, w, seeds)
    if op == "sample_weighted_hub":
        # power-law-ish: 1000 hub rows of degree 10k + filler rows
        n_hub, hub_deg = 1000, 10_000
        n = n_hub
        indptr = torch.arange(0, (n + 1) * hub_deg, hub_deg, device=device)
        indices = torch.randint(0, 1 << 20, (n * hub_deg,), device=device)
        w = torch.rand(n * hub_deg, device=device)
        seeds = torch.randint(0, n, (8192,), device=device)
        return (indptr, indices, w, seeds)
    raise SystemExit(f"unknown op {op}")


def seg_bwd_inputs(layer, dtype, device):
    """Segment-mean backward at the flagship's layer-1 shape (164k source
    rows, 16.3k targets, 163k edges of hops 1-2) or layer-2 shape (16.3k
    sources, 1024 targets, 15k edges), F = 256: every source past the
    targets has one in-edge and the remaining edges land anywhere, which
    gives the batch's mean in-degree of about 1.1."""
    torch.manual_seed(0)
    n_src, n_tgt, E = ((164_000, 16_300, 163_000) if layer == 1
                       else (16_300, 1024, 15_000))
    F = 256
    E = max(E, n_src - n_tgt)
    tgt = torch.sort(torch.randint(0, n_tgt, (E,), device=device))[0]
    col = torch.cat([torch.arange(n_tgt, n_src, device=device),
                     torch.randint(0, n_src, (E - (n_src - n_tgt),),
                                   device=device)])
    col = col[torch.randperm(E, device=device)]
    from glt_amd.ops.segment import _boundaries
    off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
    dy = torch.randn(n_tgt, 2 * F, device=device).to(dtype)
    mask = torch.randn(n_src, F, device=device).relu_().to(dtype)
    return dy, tgt, col, off, n_src, mask


def seg_bwd_table(device, iters, warmup):
    """--op seg_bwd: the atomic chain (zero fill + atomics, cast to dy's
    dtype, threshold_backward) against the gather chain (index build +
    one kernel) of segment_mean_cat's backward, deterministic mode, and
    the two halves of the gather chain on their own.  us per call from
    device events over --iters calls."""
    from glt_amd import _C

    def timed(fn):
        for _ in range(warmup):
            fn()
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    for layer in (1, 2):
        for dtype in (torch.bfloat16, torch.float32):
            dy, tgt, col, off, n_src, mask = seg_bwd_inputs(layer, dtype,
                                                            device)
            F, sz = mask.size(1), mask.element_size()

            def atomic():
                dx = _C.segment_mean_cat_bwd(dy, col, off, n_src, True)
                if dx.dtype != dtype:
                    dx = dx.to(dtype)
                return torch.ops.aten.threshold_backward(dx, mask, 0)

            def index():
                return _C.segment_transpose(col, n_src, tgt)

            src_off, in_tgt = index()

            def kernel():
                return _C.segment_mean_cat_bwd_gather(
                    dy, col, off, n_src, True, src_off, in_tgt, mask)

            def gather():
                so, it = index()
                return _C.segment_mean_cat_bwd_gather(
                    dy, col, off, n_src, True, so, it, mask)

            assert torch.equal(atomic(), gather())
            # the kernel reads dy, the mask and the index, writes dx once
            nbytes = (dy.numel() + 2 * n_src * F) * sz + \
                8 * (col.numel() + n_src + 1 + off.numel())
            t_k = timed(kernel)
            name = "L%d %s" % (layer, "bf16" if sz == 2 else "fp32")
            print(f"seg_bwd {name}: atomic chain {timed(atomic):.1f} us, "
                  f"gather chain {timed(gather):.1f} us (index "
                  f"{timed(index):.1f} us, kernel {t_k:.1f} us = "
                  f"{nbytes / 1e6:.1f} MB at {nbytes / t_k / 1e6:.2f} TB/s)")


def gatv2_table(device, iters, warmup, rounds=5):
    """--op gatv2: GATv2 attention forward + backward (all four gradients)
    at the gat_fused flagship shape, fused kernels against the torch
    composition, fp32 and bf16.  The two are timed alternately, `rounds`
    times `iters` calls each, from device events; median and range of the
    rounds, ms per call.  Then the backward's parts: the by-source index
    build, the native backward with and without the by-source pass."""
    from glt_amd import _C
    from glt_amd.ops import gatv2_composition, gatv2_softmax_aggregate
    from glt_amd.ops.segment import _offsets

    def timed(fn):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    def spread(ts):
        ts = sorted(ts)
        return "%.3f ms (%.3f - %.3f)" % (ts[len(ts) // 2], ts[0], ts[-1])

    h32, att, tgt, src, n_tgt = build_flagship_shapes("gat_fused", device)
    n_src, H, C = h32.shape
    cnt = torch.bincount(src, minlength=n_src)
    print(f"gatv2 shape: n_src {n_src}, n_tgt {n_tgt}, E {src.numel()}, "
          f"H {H}, C {C}; edges per target: median "
          f"{int(torch.bincount(tgt, minlength=n_tgt).median())}, max "
          f"{int(torch.bincount(tgt, minlength=n_tgt).max())}; in-edges per "
          f"source: median {int(cnt.median())}, median of sources with "
          f"edges {int(cnt[cnt > 0].median())}, max {int(cnt.max())}, "
          f"{int((cnt == 0).sum())} sources without edges")
    hr32 = torch.randn(n_tgt, H, C, device=device)
    g32 = torch.randn(n_tgt, H, C, device=device)
    off = _offsets(tgt, n_tgt)
    for dtype in (torch.float32, torch.bfloat16):
        name = "bf16" if dtype == torch.bfloat16 else "fp32"
        hl = h32.to(dtype).requires_grad_(True)
        hr = hr32.to(dtype).requires_grad_(True)
        at = att.clone().requires_grad_(True)
        dout = g32.to(dtype)

        def step(fn):
            hl.grad = hr.grad = at.grad = None
            fn(hr, hl, at, tgt, src, n_tgt, 0.2).backward(dout)

        fused = lambda: step(gatv2_softmax_aggregate)
        comp = lambda: step(gatv2_composition)
        for _ in range(warmup):
            fused()
            comp()
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(fused))
            tc.append(timed(comp))
        print(f"gatv2 {name} fwd+bwd: fused {spread(tf)}, composition "
              f"{spread(tc)}, ratio of medians "
              f"{sorted(tc)[rounds // 2] / sorted(tf)[rounds // 2]:.2f}x")

        with torch.no_grad():
            hl_, hr_ = hl.detach(), hr.detach()
            out, m, z, o32 = _C.gatv2_fwd(hr_, hl_, att, src, off, n_tgt,
                                          0.2, True)
            so, ie = _C.segment_transpose(src, n_src, None)
            fwd = lambda: _C.gatv2_fwd(hr_, hl_, att, src, off, n_tgt, 0.2,
                                       True)
            index = lambda: _C.segment_transpose(src, n_src, None)
            both = lambda: _C.gatv2_bwd(hr_, hl_, att, tgt, src, off, o32,
                                        m, z, dout, 0.2, so, ie)
            by_tgt = lambda: _C.gatv2_bwd(hr_, hl_, att, tgt, src, off,
                                          o32, m, z, dout, 0.2)
            parts = {"forward": fwd, "index build": index,
                     "backward, both passes": both,
                     "backward, by-target pass only (no p/ds stores)":
                         by_tgt}
            for fn in parts.values():
                for _ in range(warmup):
                    fn()
            for label, fn in parts.items():
                print(f"gatv2 {name} {label}: "
                      f"{spread([timed(fn) for _ in range(rounds)])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", required=True,
                    choices=["seg_mean", "seg_mean_cat", "gat_fused",
                             "gat_fused_bwd",
                             "mfma_gemm", "gather", "sample",
                             "sample_weighted", "sample_weighted_nr",
                             "sample_weighted_hub", "gemm_bt_bf16",
                             "gemm_kt_bf16", "seg_mean_cat_bf16",
                             "seg_wsum", "seg_wsum_bf16", "gcn_conv",
                             "gcn_conv_composite", "seg_max", "seg_max_cat",
                             "sage_conv_max", "sage_conv_max_composite",
                             "seg_bwd", "gatv2"])
    ap.add_argument("--bf16", action="store_true",
                    help="gcn_conv, seg_mean, seg_max and sage_conv_max "
                         "ops: bf16 input at F=100 (default fp32 at F=256)")
    ap.add_argument("--fwd-only", action="store_true",
                    help="seg_max ops: time the forward kernel alone (with "
                         "the arg store) instead of forward + backward")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "microbench needs a GPU"
    device = torch.device("cuda", 0)
    import glt_amd
    from glt_amd import _C

    if args.op == "seg_bwd":
        seg_bwd_table(device, args.iters, args.warmup)
        return
    if args.op == "gatv2":
        gatv2_table(device, args.iters, args.warmup)
        return
    inp = build_flagship_shapes(args.op, device, args.bf16)

    op = args.op
    if args.op == "seg_mean":
        from glt_amd.ops.segment import _boundaries
        x, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        fn = lambda: _C.segment_mean_fwd(x, src, off, n_tgt)
    elif args.op == "seg_mean_cat":
        from glt_amd.ops.segment import _boundaries
        x, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        fn = lambda: _C.segment_mean_cat_fwd(x, src, off, n_tgt)
    elif args.op == "gat_fused":
        from glt_amd.ops.segment import _boundaries
        h, att, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        fn = lambda: _C.gat_fused_fwd(h, h, att, att, src, off, 0.2)
    elif args.op == "gat_fused_bwd":
        # the backward alone, on saved forward outputs; h_tgt is cut to
        # the rows the kernels read, so that the call zero-fills one
        # [n_src, H, C] arena, not two
        from glt_amd.ops.segment import _boundaries
        h, att, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        ht = h[:n_tgt]
        out, m, z, spre = _C.gat_fused_fwd(ht, h, att, att, src, off, 0.2)
        dout = torch.randn_like(out)
        fn = lambda: _C.gat_fused_bwd(ht, h, att, att, src, off, out, m, z,
                                      spre, dout, 0.2)
    elif args.op == "mfma_gemm":
        A, B = inp
        fn = lambda: _C.sage_gemm(A, B, None, False)
    elif args.op == "gemm_bt_bf16":
        A, W, b = inp
        fn = lambda: _C.gemm_bt_bf16(A, W, b, True, False)
    elif args.op == "gemm_kt_bf16":
        A, B = inp
        fn = lambda: _C.gemm_kt_bf16(A, B, True)
    elif args.op == "seg_mean_cat_bf16":
        from glt_amd.ops.segment import _boundaries
        x, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        fn = lambda: _C.segment_mean_cat_fwd(x, src, off, n_tgt)
    elif args.op in ("seg_wsum", "seg_wsum_bf16"):
        # forward kernel with all three factors (the GCN aggregation)
        from glt_amd.ops.segment import _boundaries
        x, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        w = torch.rand(src.numel(), device=device)
        a = torch.rand(n_tgt, device=device)
        b = torch.rand(x.size(0), device=device)
        fn = lambda: _C.segment_wsum_fwd(x, src, off, w, a, b)
    elif args.op in ("seg_max", "seg_max_cat"):
        # forward (with the arg store) + backward, as in a training step
        from glt_amd.ops.segment import _boundaries
        x, tgt, src, n_tgt = inp
        off = torch.searchsorted(tgt, _boundaries(n_tgt, device))
        cat = args.op == "seg_max_cat"
        F = x.size(1)
        dy = torch.randn(n_tgt, 2 * F if cat else F,
                         device=device).to(x.dtype)
        fwd = lambda: _C.segment_ext_fwd(x, src, off, n_tgt, True, cat, True)
        sz = x.element_size()
        print(f"forward bytes (E*F*{sz} + E*8 + n_tgt*F*({sz}+4)): "
              f"{src.numel() * (F * sz + 8) + n_tgt * F * (sz + 4)}")
        if args.fwd_only:
            fn = fwd
        else:
            def fn():
                _, arg = fwd()
                _C.segment_ext_bwd(dy, arg, x.size(0), cat, False)
    elif args.op in ("sage_conv_max", "sage_conv_max_composite"):
        # SAGEConv(aggr='max') forward + backward with the gradient of x:
        # fused kernels against the torch composition
        from glt_amd.models.layers import SAGEConv
        x, tgt, src, n_tgt = inp
        x.requires_grad_(True)
        conv = SAGEConv(x.size(1), 256, aggr="max").to(device)
        ei = torch.stack([tgt, src])
        fused = args.op == "sage_conv_max"
        gy = torch.randn(n_tgt, 256, device=device).to(x.dtype)

        def fn():
            conv.zero_grad(set_to_none=True)
            x.grad = None
            conv(x, ei, n_tgt, sorted_by_target=fused).backward(gy)
    elif args.op in ("gcn_conv", "gcn_conv_composite"):
        # GCNConv forward + backward (weight gradient only, as in layer
        # 1): fused aggregation against the torch composition
        from glt_amd.models.layers import GCNConv
        x, tgt, src, n_tgt = inp
        conv = GCNConv(x.size(1), 256).to(device)
        ei = torch.stack([tgt, src])
        fused = args.op == "gcn_conv"
        gy = torch.randn(n_tgt, 256, device=device).to(x.dtype)

        def fn():
            conv.zero_grad(set_to_none=True)
            conv(x, ei, n_tgt, sorted_by_target=fused).backward(gy)
    elif args.op == "gather":
        feats, rows = inp
        store = _C.UnifiedFeatureStore(0)
        store.append(feats)
        fn = lambda: store.gather(rows)
    elif op == "sample":
        indptr, indices, seeds = inp
        fn = lambda: _C.sample_neighbors(indptr, indices, seeds, 15)
    else:  # weighted variants
        indptr, indices, w, seeds = inp
        rep = op != "sample_weighted_nr"
        fn = lambda: _C.sample_neighbors(indptr, indices, seeds, 15,
                                         edge_weights=w, weighted=True,
                                         replace=rep)

    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    print(f"{args.op}: {dt * 1e6:.1f} us/iter over {args.iters} iters")


if __name__ == "__main__":
    main()

"""GAT v1 attention kernels (hip_gat.hip) on their own: _C.gat_fused_fwd /
_C.gat_fused_bwd, _C.gat_multi_fwd / _C.gat_multi_bwd and
ops.gat_softmax_aggregate.

Edges sorted by target, t = tgt[e], s = src[e]; h_tgt [Nt.., H, C], h_src
[Ns, H, C], att_src and att_dst [H, C] (the header of hip_gat.hip):

    spre_e    = <h_tgt[t,h], att_dst[h]> + <h_src[s,h], att_src[h]>
    score_e   = leaky_relu(spre_e, slope)
    p_e       = softmax over seg(t) of score_e
    out[t,h]  = sum_{e in seg(t)} p_e * h_src[s,h]          (empty: 0)
    ds_e      = p_e * (<dout_t, h_src_s> - <dout_t, out_t>) * leaky'(spre_e)
    dh_src[s] = sum_{e: src[e]=s} (p_e * dout_t + ds_e * att_src[h])
    dh_tgt[t] = (sum_{e in seg(t)} ds_e) * att_dst[h]
    datt_src[h] = sum_e ds_e * h_src[s,h]
    datt_dst[h] = sum_t (sum_{e in seg(t)} ds_e) * h_tgt[t,h]

Exact tests (torch.equal).  The single-relation entry points are the
one-relation case of the multi-relation ones and launch the same kernels, so
their forward outputs agree bit for bit; argued in each docstring.

Bounded tests.  The reference is `_formulas` in fp64 on the CPU from the
exact inputs (for bf16, the bf16-rounded inputs); gradients come from the
lines above, not from autograd.  The bound is a running error bound worked
out from the data by `_bounds`, never from what the kernels give:

    |x - ref| <= gamma * A,   gamma = (n + Delta) * 2^-23

  A      the same sum as x with every term replaced by its absolute value,
         all the way down: A_out = sum_e p_e |h_src_s|; ds_e becomes p_e *
         leaky' * (sum_c |dout_tc h_src_sc| + sum_c |dout_tc| A_out_tc), the
         two dots with absolute terms and added, not subtracted (a segment
         of one edge has ds_e = 0 exactly, and a computed one of the size
         of the dots' rounding); the gradients are their sums with that
         ds_e and |att|, |h|, |dout|.
  n      the operation count on the longest path, L + 2 C + 16: L the
         longest chain of additions into the value (deg_max for out and
         dh_tgt, deg_max + the largest in-degree for dh_src, deg_max + E
         for datt, which sums over all edges), 2 C for the two dots in a
         row (the score's, then ds_e's) taken as sequential sums, 16 for
         leaky_relu, the subtraction of the maximum, exp, the rescales of
         the online softmax, 1/Z, the products and the final rounding.
         The score's error enters p_e not as a relative but as an absolute
         one, depth * u * sum_c (|h_tgt att_dst| + |h_src att_src|), and
         that sum is up to 15 here; the count covers it because the
         kernels' wave tree and torch's vectorised sums have depth <= 9,
         not C.  The bound is a worst case all the same, one to three
         orders above what an fp32 evaluation gives (printed).
  Delta  the largest |score_e - max of its segment|: __expf(x) is
         exp2(x * log2 e), and rounding that product is a relative error of
         |x| u in the result.
  bf16   out is rounded once to bf16: 2^-8 |ref| more.  The backward takes
         <dout_t, out_t> from that rounded out, which moves ds_e by at most
         p_e * leaky' * sum_c |dout_tc| * 2^-8 |out_tc|; the gradients (fp32
         arenas) get the sums of that term in place of ds_e, B below.

leaky' jumps at spre_e = 0, so the inputs are drawn from the first seed for
which no |spre_e| lies within 4 (C + 2) u sb_e of 0 (a property of the
reference alone).  `test_bound_admits_the_fp32_composition` runs the same
formulas in fp32 on the CPU against the same bound, without a GPU: the bound
is not too tight for an honest fp32 evaluation.  Every case prints its
measured error and bound (pytest -s).
"""
import pytest
import torch

U = 2.0 ** -24          # fp32 unit roundoff; gamma uses 2 U = 2^-23
UBF = 2.0 ** -8
SLOPE = 0.2
KEYS = ("out", "dh_src", "dh_tgt", "datt_src", "datt_dst")
SEG = (0, 1, 4, 5, 37, 0, 8, 3, 2)     # edges per target of the base graph
CS = (1, 7, 64, 65, 128)
DTYPES = (torch.float32, torch.bfloat16)


# --------------------------------------------------------------------------
# the definition, its running error bound, the inputs
# --------------------------------------------------------------------------
def _formulas(ht, hs, a_s, a_d, tgt, src, n_tgt, slope, dout):
    """The header lines in the dtype of the inputs, on their device."""
    H, C = hs.shape[1:]
    z2 = lambda *s: torch.zeros(*s, dtype=hs.dtype)
    hse = hs[src]
    spre = (ht[:n_tgt] * a_d).sum(-1)[tgt] + (hs * a_s).sum(-1)[src]
    score = torch.where(spre > 0, spre, spre * slope)
    m = torch.full((n_tgt, H), float("-inf"), dtype=hs.dtype)
    m.scatter_reduce_(0, tgt.unsqueeze(1).expand_as(score), score,
                      reduce="amax")
    ex = (score - m[tgt]).exp()
    Z = z2(n_tgt, H).index_add_(0, tgt, ex)
    p = ex / Z[tgt]
    out = z2(n_tgt, H, C).index_add_(0, tgt, p.unsqueeze(-1) * hse)
    lp = torch.where(spre > 0, torch.ones_like(spre),
                     torch.full_like(spre, slope))
    ds = p * ((dout[tgt] * hse).sum(-1) - (dout * out).sum(-1)[tgt]) * lp
    dsum = z2(n_tgt, H).index_add_(0, tgt, ds)
    dh_tgt = torch.zeros_like(ht)
    dh_tgt[:n_tgt] = dsum.unsqueeze(-1) * a_d
    return dict(
        out=out, Z=Z, spre=spre, score=score, m=m, p=p, lp=lp,
        dh_src=torch.zeros_like(hs).index_add_(
            0, src, p.unsqueeze(-1) * dout[tgt] + ds.unsqueeze(-1) * a_s),
        dh_tgt=dh_tgt, datt_src=(ds.unsqueeze(-1) * hse).sum(0),
        datt_dst=(dsum.unsqueeze(-1) * ht[:n_tgt]).sum(0))


def _bounds(ref, ht, hs, a_s, a_d, tgt, src, n_tgt, dout):
    """(gamma, A, B, kink) of the module docstring from the fp64 reference
    and inputs; gamma per key, kink true where spre_e is too close to 0."""
    H, C = hs.shape[1:]
    E = tgt.numel()
    z2 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    p, lp = ref["p"], ref["lp"]
    hse, ad, ado = hs[src].abs(), dout.abs(), dout.abs()[tgt]
    A_out = z2(n_tgt, H, C).index_add_(0, tgt, p.unsqueeze(-1) * hse)

    def grads(dsb):
        dsum = z2(n_tgt, H).index_add_(0, tgt, dsb)
        dh_tgt = torch.zeros_like(ht)
        dh_tgt[:n_tgt] = dsum.unsqueeze(-1) * a_d.abs()
        return dict(
            dh_src=dsb.unsqueeze(-1) * a_s.abs(), dh_tgt=dh_tgt,
            datt_src=(dsb.unsqueeze(-1) * hse).sum(0),
            datt_dst=(dsum.unsqueeze(-1) * ht[:n_tgt].abs()).sum(0))

    A = grads(p * lp * ((ado * hse).sum(-1) + (ad * A_out).sum(-1)[tgt]))
    A["dh_src"] = torch.zeros_like(hs).index_add_(
        0, src, p.unsqueeze(-1) * ado + A["dh_src"])
    A["out"] = A_out
    B = grads(p * lp * (ad * ref["out"].abs()).sum(-1)[tgt])
    B["dh_src"] = torch.zeros_like(hs).index_add_(0, src, B["dh_src"])
    B["out"] = ref["out"].abs()
    delta = (ref["score"] - ref["m"][tgt]).abs().max().item() if E else 0.0
    deg = int(torch.bincount(tgt, minlength=1).max()) if E else 0
    indeg = int(torch.bincount(src, minlength=1).max()) if E else 0
    L = dict(out=deg, dh_tgt=deg, dh_src=deg + indeg, datt_src=deg + E,
             datt_dst=deg + E)
    gamma = {k: (L[k] + 2 * C + 16 + delta) * 2 * U for k in KEYS}
    sb = ((ht[:n_tgt] * a_d).abs().sum(-1)[tgt]
          + (hs * a_s).abs().sum(-1)[src])
    kink = ref["spre"].abs() <= 4 * (C + 2) * 2 * U * sb
    return gamma, A, B, kink


class Case:
    """Inputs on the CPU in `dtype` (att fp32), fp64 reference and bounds."""

    def __init__(self, seg, n_src, H, C, dtype, extra_tgt_rows=3, salt=0):
        n_tgt = len(seg)
        tgt = torch.repeat_interleave(torch.arange(n_tgt),
                                      torch.as_tensor(seg))
        E = tgt.numel()
        for seed in range(64):
            g = torch.Generator().manual_seed(1000 * C + 64 * salt + seed)
            r = lambda *s: torch.randn(*s, generator=g)
            self.ht = r(n_tgt + extra_tgt_rows, H, C).to(dtype)
            self.hs = r(n_src, H, C).to(dtype)
            # scores of a few units whatever C is
            self.a_s = 2 * r(H, C) / C ** 0.5
            self.a_d = 2 * r(H, C) / C ** 0.5
            self.dout = r(n_tgt, H, C).to(dtype)
            src = torch.randint(0, n_src, (E,), generator=g)
            if E > 1:
                src[1::7] = src[0:-1:7]  # repeats next to each other
            self.src, self.tgt, self.n_tgt = src, tgt, n_tgt
            self.off = torch.searchsorted(tgt, torch.arange(n_tgt + 1))
            d = [v.double() for v in (self.ht, self.hs, self.a_s, self.a_d)]
            self.ref = _formulas(*d, tgt, src, n_tgt, SLOPE,
                                 self.dout.double())
            self.gamma, self.A, self.B, kink = _bounds(
                self.ref, *d, tgt, src, n_tgt, self.dout.double())
            if not kink.any():
                break
        else:
            raise AssertionError("no seed keeps spre off the kink")
        self.bf16 = dtype == torch.bfloat16
        self.H, self.C = H, C

    def check(self, name, got, keys=KEYS, A_extra=None):
        """got[k] within gamma * A[k] (+ 2^-8 B[k] for bf16) of ref[k]."""
        for k in keys:
            bound = self.gamma[k] * self.A[k]
            if A_extra is not None and k in A_extra:
                bound = bound + A_extra[k]
            if self.bf16:
                bound = bound + UBF * self.B[k]
            err = (got[k].detach().double().cpu() - self.ref[k]).abs()
            ratio = (err / bound.clamp(min=1e-300)).max().item() \
                if err.numel() else 0.0
            print("%s %s: max err %.3e, max bound %.3e, max err/bound %.3f"
                  % (name, k, err.max().item() if err.numel() else 0.0,
                     bound.max().item() if bound.numel() else 0.0, ratio))
            assert torch.isfinite(got[k]).all(), (name, k)
            assert (err <= bound).all(), (name, k, ratio)

    def cuda(self):
        return tuple(v.cuda() for v in (self.ht, self.hs, self.a_s, self.a_d,
                                        self.src, self.off))


_cases = {}


def _base(C, dtype):
    key = ("base", C, dtype)
    if key not in _cases:
        _cases[key] = Case(SEG, 23, 2, C, dtype)
    return _cases[key]


# n_tgt * H = 18, 6000, 18000: the backward's split S = 8, 5, 1
SPLITS = {18: 8, 6000: 5, 18000: 1}


def _split(n_items):
    key = ("split", n_items)
    if key not in _cases:
        n_tgt = n_items // 2
        seg = [1 + (t % 2) for t in range(n_tgt)]  # one or two edges
        _cases[key] = Case(seg, n_tgt + 11, 2, 8, torch.float32, 0)
    return _cases[key]


def _fwd_bwd(case):
    """The single-relation kernels on the case: dict of KEYS, m, Z, spre."""
    from glt_amd import _C

    ht, hs, a_s, a_d, src, off = case.cuda()
    out, m, z, spre = _C.gat_fused_fwd(ht, hs, a_s, a_d, src, off, SLOPE)
    dht, dhs, das, dad = _C.gat_fused_bwd(ht, hs, a_s, a_d, src, off, out, m,
                                          z, spre, case.dout.cuda(), SLOPE)
    return dict(out=out, m=m, Z=z, spre=spre, dh_tgt=dht, dh_src=dhs,
                datt_src=das, datt_dst=dad)


# --------------------------------------------------------------------------
# CPU: the bound admits an honest fp32 evaluation
# --------------------------------------------------------------------------
def _composition32(case):
    f = lambda v: v.float()
    return _formulas(f(case.ht), f(case.hs), case.a_s, case.a_d, case.tgt,
                     case.src, case.n_tgt, SLOPE, f(case.dout))


@pytest.mark.parametrize("C", CS)
def test_bound_admits_the_fp32_composition(C):
    """The formulas in fp32 torch ops on the CPU stay inside the bound the
    kernels are held to: it is not too tight.  It is not vacuous either:
    gamma stays below 5e-5, so that no bound exceeds 5e-5 of the sum of
    the absolute terms of the value it bounds."""
    case = _base(C, torch.float32)
    assert max(case.gamma.values()) < 5e-5
    case.check("composition C=%d" % C, _composition32(case))


@pytest.mark.parametrize("n_items", list(SPLITS))
def test_bound_admits_the_fp32_composition_split_shapes(n_items):
    case = _split(n_items)
    case.check("composition n_tgt*H=%d" % n_items, _composition32(case))


# --------------------------------------------------------------------------
# GPU: bounded against fp64
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_single_within_running_bound(C, dtype):
    """The base graph: empty segments at the start and in the middle, one
    exact 4-edge batch, a batch plus a tail, a 37-edge hub whose S = 8
    slices are uneven (5 + 5 + ... + 2), short segments whose later slices
    are empty; C of one lane, odd, one full pass, a second pass of one
    lane, two full passes.

    Exact: an empty target gets out = 0, Z = 0 and a zero dh_tgt row; the
    h_tgt rows at and past n_tgt get zero gradient."""
    case = _base(C, dtype)
    got = _fwd_bwd(case)
    assert got["out"].dtype == dtype
    case.check("single C=%d %s" % (C, dtype), got)
    empty = [t for t, n in enumerate(SEG) if n == 0]
    assert not got["out"][empty].any()
    assert not got["Z"][empty].any()
    assert not got["dh_tgt"][empty].any()
    assert not got["dh_tgt"][case.n_tgt:].any()
    err = (got["spre"].double().cpu() - case.ref["spre"]).abs().max().item()
    print("spre max err %.3e" % err)


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", list(SPLITS))
def test_backward_split_sizes(n_items):
    """n_tgt * H = 18, 6000, 18000 waves: the backward splits each segment
    S = 8, 5, 1 ways (32768 / (n_tgt * H), clamped to [1, 8]); with one or
    two edges per target all but the first one or two sub-waves of a
    segment get an empty slice."""
    assert max(1, min(8, 32768 // n_items)) == SPLITS[n_items]
    case = _split(n_items)
    case.check("split n_tgt*H=%d" % n_items, _fwd_bwd(case))


@pytest.mark.gpu
def test_autograd_wrapper_runs_the_same_kernels():
    """ops.gat_softmax_aggregate returns gat_fused_fwd's out bit for bit
    (the forward is deterministic) and gradients inside the bound."""
    from glt_amd.ops import gat_softmax_aggregate

    case = _base(7, torch.float32)
    ht, hs, a_s, a_d, src, off = case.cuda()
    leaves = [v.clone().requires_grad_(True) for v in (ht, hs, a_s, a_d)]
    out = gat_softmax_aggregate(*leaves, case.tgt.cuda(), src, case.n_tgt,
                                SLOPE)
    out.backward(case.dout.cuda())
    assert torch.equal(out, _fwd_bwd(case)["out"])
    case.check("autograd", dict(out=out, dh_tgt=leaves[0].grad,
                                dh_src=leaves[1].grad,
                                datt_src=leaves[2].grad,
                                datt_dst=leaves[3].grad))


# --------------------------------------------------------------------------
# GPU: the single path is the one-relation case of the multi path
# --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", CS)
def test_one_relation_multi_equals_single(C, dtype):
    """gat_multi_fwd with one relation, contiguous views and no bias is
    gat_fused_fwd: out, m, Z and spre are equal bit for bit.  So are they
    from row-strided views (every other row of a tensor twice as tall),
    which take the packed-table kernel instead of the one-relation one:
    both run the one device body, and a stride only moves addresses."""
    from glt_amd import _C

    case = _base(C, dtype)
    ht, hs, a_s, a_d, src, off = case.cuda()
    one = _C.gat_fused_fwd(ht, hs, a_s, a_d, src, off, SLOPE)
    multi = _C.gat_multi_fwd([ht], [hs], [a_s], [a_d], [src], [off], SLOPE,
                             [])
    every_other = lambda v: torch.repeat_interleave(v, 2, dim=0)[::2]
    assert every_other(hs).stride(0) == 2 * hs.stride(0)
    strided = _C.gat_multi_fwd([every_other(ht)], [every_other(hs)], [a_s],
                               [a_d], [src], [off], SLOPE, [])
    for name, a, b, c in zip(("out", "m", "Z", "spre"), one, multi, strided):
        assert torch.equal(a, b), name
        assert torch.equal(a, c), name


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_four_relations_strided_views(dtype):
    """Four relations in one launch: different n_tgt (9, 0 edges on 4
    targets, 5, 9), h views that are column slices of a wider tensor (row
    stride 3 H C, not H C), the last relation with a bias.

    Each of the first three relations' slices of the arenas equals
    gat_fused_fwd on that relation's contiguous copy bit for bit: the
    stride only moves addresses.  The biased relation's out is within the
    running bound (+ u |bias|, the rounding of the added bias) of the fp64
    reference + bias.  The backward writes into column slices of one arena
    per side; each relation's slice is within the bound, and the columns
    and rows no relation owns stay zero."""
    from glt_amd import _C

    H, C = 2, 7
    cases = [Case(SEG, 23, H, C, dtype),
             Case((0, 0, 0, 0), 23, H, C, dtype),
             Case((3, 0, 6, 1, 2), 23, H, C, dtype, salt=1),
             Case(SEG, 23, H, C, dtype, salt=2)]
    R, W = len(cases), 3 * H * C
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(H * C, generator=g)
    wide_t = torch.zeros(R, 12, W, dtype=dtype)
    wide_s = torch.zeros(R, 23, W, dtype=dtype)
    for r, c in enumerate(cases):
        wide_t[r, :c.ht.size(0), H * C:2 * H * C] = c.ht.reshape(-1, H * C)
        wide_s[r, :, H * C:2 * H * C] = c.hs.reshape(-1, H * C)
    wide_t, wide_s = wide_t.cuda(), wide_s.cuda()
    view = lambda w, r, n: w[r, :n, H * C:2 * H * C].view(n, H, C)
    hts = [view(wide_t, r, c.ht.size(0)) for r, c in enumerate(cases)]
    hss = [view(wide_s, r, 23) for r in range(R)]
    assert hts[0].stride(0) == W and not hts[0].is_contiguous()
    dev = [c.cuda() for c in cases]
    a_s, a_d = [d[2] for d in dev], [d[3] for d in dev]
    srcs, offs = [d[4] for d in dev], [d[5] for d in dev]
    empty = torch.empty(0, device="cuda")
    out, m, z, spre = _C.gat_multi_fwd(
        hts, hss, a_s, a_d, srcs, offs, SLOPE,
        [empty, empty, empty, bias.cuda()])
    nt = [c.n_tgt for c in cases]
    ne = [c.src.numel() for c in cases]
    outs, ms, zs = (torch.split(v, nt) for v in (out, m, z))
    spres = torch.split(spre, ne)
    for r in range(3):
        one = _C.gat_fused_fwd(*dev[r], SLOPE)
        for name, a, b in zip(("out", "m", "Z", "spre"), one,
                              (outs[r], ms[r], zs[r], spres[r])):
            assert torch.equal(a, b), (r, name)
    assert not outs[1].any() and not zs[1].any()
    c3 = cases[3]
    got = outs[3].double().cpu() - bias.double().view(H, C)
    c3.check("biased relation", dict(out=got), keys=("out",),
             A_extra=dict(out=(2 * U + (UBF if c3.bf16 else 0))
                          * bias.double().abs().view(H, C).expand(
                              c3.n_tgt, H, C)))

    dout = torch.cat([c.dout for c in cases]).cuda()
    dt_arena = torch.zeros(R, 12, W, device="cuda")
    ds_arena = torch.zeros(R, 23, W, device="cuda")
    das = torch.zeros(R, H, C, device="cuda")
    dad = torch.zeros(R, H, C, device="cuda")
    _C.gat_multi_bwd(
        hts, hss, a_s, a_d, srcs, offs, out, m, z, spre, dout,
        [view(dt_arena, r, c.ht.size(0)) for r, c in enumerate(cases)],
        [view(ds_arena, r, 23) for r in range(R)], list(das), list(dad),
        SLOPE)
    for r, c in enumerate(cases[:3]):
        c.check("relation %d" % r, dict(
            dh_tgt=view(dt_arena, r, c.ht.size(0)),
            dh_src=view(ds_arena, r, 23), datt_src=das[r], datt_dst=dad[r]),
            keys=KEYS[1:])
    for arena in (dt_arena, ds_arena):
        assert not arena[:, :, :H * C].any()
        assert not arena[:, :, 2 * H * C:].any()
    assert not dt_arena[1].any() and not ds_arena[1].any()
    assert not dt_arena[2, 5:].any()

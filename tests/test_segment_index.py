"""The batch's index structures: _C.segment_offsets (CSR offsets of the
ascending targets in one streaming pass) against torch.searchsorted, and
_C.segment_transpose (the inverted index, a counting sort) against
torch.sort(stable=True) plus searchsorted and against its own rocprim-sort
path (GLT_SEGMENT_INDEX=sort), tensor for tensor.
"""
import pytest
import torch

from glt_amd import _C
from glt_amd.ops import segment as seg_ops

pytestmark = pytest.mark.gpu


def _dev(values):
    return torch.as_tensor(values, dtype=torch.long, device="cuda")


def _rand(lo, hi, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (n,), generator=g).cuda()


# --------------------------------------------------------------------------
# segment_offsets
# --------------------------------------------------------------------------
def _offset_case(name):
    if name == "no_edges":
        return _dev([]), 9
    if name == "no_targets":
        return _dev([]), 0
    if name == "empty_head_middle_tail":
        # targets 0-2, 6-9 and 13-19 own nothing
        return _dev([3, 3, 4, 5, 5, 5, 10, 11, 11, 12]), 20
    if name == "one_target_owns_all":
        return torch.full((777,), 5, dtype=torch.long, device="cuda"), 9
    if name == "random_3000_over_700":
        return torch.sort(_rand(0, 700, 3000, 21))[0], 700
    raise AssertionError(name)


@pytest.mark.parametrize("name", [
    "no_edges", "no_targets", "empty_head_middle_tail",
    "one_target_owns_all", "random_3000_over_700"])
def test_offsets_equal_searchsorted(name):
    tgt, n_tgt = _offset_case(name)
    want = torch.searchsorted(tgt, torch.arange(n_tgt + 1, device="cuda"))
    got = _C.segment_offsets(tgt, n_tgt)
    assert got.dtype == torch.long and got.shape == (n_tgt + 1,)
    assert torch.equal(got, want)
    assert int(got[-1]) == tgt.numel()
    # the op layer takes the kernel on the device, searchsorted on the CPU
    assert torch.equal(seg_ops._offsets(tgt, n_tgt), want)
    assert torch.equal(seg_ops._offsets(tgt.cpu(), n_tgt), want.cpu())


# --------------------------------------------------------------------------
# segment_transpose
# --------------------------------------------------------------------------
def _transpose_case(name):
    if name == "no_edges":
        return _dev([]), 6
    if name == "one_edge":
        return _dev([4]), 6
    if name == "one_source_5000":
        return torch.zeros(5000, dtype=torch.long, device="cuda"), 1
    if name == "gaps_head_and_tail":
        return _rand(100, 900, 3000, 22), 1000
    if name == "random_3000_over_700":
        return _rand(0, 700, 3000, 23), 700
    if name == "lists_of_64_and_65":
        # source 3 gets exactly 64 edges, source 8 exactly 65, spread over
        # the edge order among 500 edges of other sources
        col = _rand(10, 40, 629, 24)
        spots = torch.randperm(629, generator=torch.Generator()
                               .manual_seed(25)).cuda()
        col[spots[:64]] = 3
        col[spots[64:129]] = 8
        return col, 40
    raise AssertionError(name)


@pytest.mark.parametrize("name", [
    "no_edges", "one_edge", "one_source_5000", "gaps_head_and_tail",
    "random_3000_over_700", "lists_of_64_and_65"])
def test_transpose_equals_stable_sort_and_sort_path(name, monkeypatch):
    col, n_src = _transpose_case(name)
    E = col.numel()
    if name == "lists_of_64_and_65":
        assert int((col == 3).sum()) == 64 and int((col == 8).sum()) == 65
    keys, want_idx = torch.sort(col, stable=True)
    want_off = torch.searchsorted(keys, torch.arange(n_src + 1,
                                                     device="cuda"))
    tgt = torch.sort(_rand(0, 400, E, 26))[0]

    monkeypatch.delenv("GLT_SEGMENT_INDEX", raising=False)
    off, idx = _C.segment_transpose(col, n_src)
    off_t, in_tgt = _C.segment_transpose(col, n_src, tgt)
    assert off.dtype == torch.long and off.shape == (n_src + 1,)
    assert idx.dtype == torch.long and idx.shape == (E,)
    assert torch.equal(off, want_off) and torch.equal(off_t, want_off)
    assert torch.equal(idx, want_idx)           # ascending e within a list
    assert torch.equal(in_tgt, tgt[want_idx])

    monkeypatch.setenv("GLT_SEGMENT_INDEX", "sort")
    s_off, s_idx = _C.segment_transpose(col, n_src)
    s_off_t, s_in_tgt = _C.segment_transpose(col, n_src, tgt)
    assert torch.equal(s_off, off) and torch.equal(s_idx, idx)
    assert torch.equal(s_off_t, off_t) and torch.equal(s_in_tgt, in_tgt)

"""The device build of a sparse index's term-major twin (zvk_sparse_invb.hip.h), checked without a GPU on the two numpy models of
tests/sparse_inv_build_ref.py: the radix scheme (digit passes from the OR of the indices, per-block histograms, one scan, a stable
scatter) gives the arrays of the stable argsort for every case tests/test_gpu_sparse_inverted_build.py builds, at several block
sizes, so the arrays the GPU is held to are known to be right before any GPU sees them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_inv_build_ref as M  # noqa: E402

BLOCKS = [64, 256, 2048]
DTYPES = ["fp32", "fp16"]


def _check_twin(case, twin):
    counts, indices, values = case
    terms, list_off, ppos, pval = twin
    E = indices.size
    assert terms.dtype == np.uint32 and list_off.dtype == np.uint64 and ppos.dtype == np.uint32
    assert pval.dtype == (np.uint16 if values.dtype.itemsize == 2 else np.uint32)
    assert np.array_equal(terms, np.unique(indices))
    assert list_off.size == terms.size + 1 and list_off[0] == 0 and list_off[-1] == E
    assert np.all(list_off[1:] > list_off[:-1]) or E == 0
    assert ppos.size == E and pval.size == E
    off = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    vraw = M.raw(values)
    for t in range(terms.size):
        p = ppos[int(list_off[t]):int(list_off[t + 1])].astype(np.int64)
        assert np.all(p[1:] > p[:-1])                                  # a row holds an index once: strictly ascending
    # every posting is the stored element it came from
    for j in range(0, E, max(1, E // 200)):
        t = int(np.searchsorted(list_off, j, side="right")) - 1
        r = int(ppos[j])
        run = indices[off[r]:off[r + 1]]
        at = int(np.searchsorted(run, terms[t]))
        assert run[at] == terms[t] and vraw[off[r] + at] == pval[j]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("block", BLOCKS)
def test_radix_scheme_equals_stable_argsort_on_every_case(block, dtype):
    for name, case in M.all_cases(block, dtype).items():
        want = M.twin_model(*case)
        got, passes = M.radix_model(*case, block)
        assert M.same_twin(got, want), name
        assert passes == M.passes_of(case[1]), name
        _check_twin(case, want)


@pytest.mark.parametrize("block", BLOCKS)
def test_single_list_keeps_position_order(block):
    case = M.single_list_case(block, "fp32")
    terms, list_off, ppos, pval = M.radix_model(*case, block)[0]
    assert terms.tolist() == [77] and list_off.tolist() == [0, 2 * block + 5]
    assert np.array_equal(ppos, np.arange(2 * block + 5, dtype=np.uint32))
    assert pval.tobytes() == M.raw(case[2]).tobytes()


@pytest.mark.parametrize("block", BLOCKS)
def test_alternating_indices_share_the_low_byte(block):
    counts, indices, values = M.alternating_case(block, "fp16")
    assert len({int(i) & 255 for i in indices}) == 1 and len({(int(i) >> 8) & 255 for i in indices}) == 2
    terms, list_off, ppos, pval = M.radix_model(counts, indices, values, block)[0]
    n = counts.size
    assert terms.tolist() == [0x0105, 0x0305]
    assert np.array_equal(ppos[:int(list_off[1])], np.arange(1, n, 2, dtype=np.uint32))
    assert np.array_equal(ppos[int(list_off[1]):], np.arange(0, n, 2, dtype=np.uint32))


def test_pass_counts():
    for name, _, want in M.PASS_CASES:
        case, w = M.pass_case(name, "fp32")
        assert w == want and M.passes_of(case[1]) == want, name
        assert M.radix_sort_order(case[1], 256)[1] == want
    assert M.passes_of(np.zeros(0, np.uint32)) == 0
    case = M.zero_low_digit_case("fp32")
    assert not np.any(case[1] & 255) and int(case[1].max()) < 65536 and M.passes_of(case[1]) == 2
    assert M.same_twin(M.radix_model(*case, 256)[0], M.twin_model(*case))


def test_values_are_moved_as_bits():
    for dtype in DTYPES:
        case = M.edge_case(3 * 64 + 17, dtype)
        v = M.raw(case[2])
        zero = np.uint16(0x8000) if dtype == "fp16" else np.uint32(0x80000000)
        assert np.any(v == zero)                                       # -0.0 is among the values
        exp = np.uint16(0x7c00) if dtype == "fp16" else np.uint32(0x7f800000)
        assert np.any(((v & exp) == 0) & ((v & ~zero & ~exp) != 0))    # and so are denormals
        pval = M.twin_model(*case)[3]
        assert np.array_equal(np.sort(pval), np.sort(v))


def test_empty_twins():
    for case in (M.empty_rows_case("fp32"), M.no_rows_case("fp16")):
        for twin in (M.twin_model(*case), M.radix_model(*case, 256)[0]):
            terms, list_off, ppos, pval = twin
            assert terms.size == 0 and list_off.tolist() == [0] and ppos.size == 0 and pval.size == 0


def test_ragged_case_has_its_edges():
    B = 2048
    counts, indices, values = M.ragged_case(B, "fp32")
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    long_row = int(np.nonzero(counts == 300)[0][0])
    assert off[long_row] < B < off[long_row + 1]                       # the long row spans the first block boundary
    assert counts[-1] == 0 and np.any(counts[:long_row] == 0)

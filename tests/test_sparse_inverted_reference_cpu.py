"""The premises of the inverted-list search of sparse rows (zvec_hip_sparse_set_inverted, zvk_sparse_inv.hip.h), checked without a GPU
on a numpy model of the twin: a STABLE sort of the stored elements by index.  Because the elements stand in position order in the
CSR arrays, every posting list then ascends by position, so positions inside a list are distinct (the kernel's race-freedom) and a
tile's share of a list is one contiguous range between two lower bounds.  Term-at-a-time fp32 accumulation over the model, whole
or tile by tile, reproduces tests/sparse_ref.py's fp64 reference within its band B = (m + 1) * 2^-23 * A, which is derived for
any order of summation: the band the GPU test holds the kernel to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402

CASES = [(1000, 65, 50, False), (1000, 65, 100000, True), (5000, 63, 50, False), (5000, 64, 100000, True), (65, 64, 100000, True),
         (1, 63, 100000, True)]


def build_twin(rows):
    """terms (distinct indices, ascending), list_off [nterms + 1], ppos, pval: the model of the library's host build"""
    counts, idx, val = rows
    pos = np.repeat(np.arange(len(counts), dtype=np.uint32), np.asarray(counts, np.int64))
    order = np.argsort(idx, kind="stable")
    terms, starts = np.unique(idx[order], return_index=True)
    list_off = np.concatenate([starts, [idx.size]]).astype(np.int64)
    return terms.astype(np.uint32), list_off, pos[order], np.asarray(val)[order]


def fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product is exact in fp64 (24 x 24 bits); the sum is rounded to fp64, then to fp32"""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def term_at_a_time(twin, queries, n, tile=None):
    """[nq][n] fp32 scores: per query one accumulator per position, the query's terms in run order, each walking its list (tile:
    only between the lower bounds of the tile's two ends, tile after tile, as the kernel's work items do)"""
    terms, list_off, ppos, pval = twin
    qc, qi, qv = queries
    qo = R.offsets(qc)
    out = np.zeros((len(qc), n), np.float32)
    tiles = [(0, n)] if tile is None else [(t, min(n, t + tile)) for t in range(0, n, tile)]
    for q in range(len(qc)):
        acc = np.zeros(n, np.float32)
        for t0, t1 in tiles:
            for e in range(qo[q], qo[q + 1]):
                at = int(np.searchsorted(terms, qi[e]))
                if at == terms.size or terms[at] != qi[e]:
                    continue                                       # an absent term is skipped
                lo, hi = int(list_off[at]), int(list_off[at + 1])
                s = lo + int(np.searchsorted(ppos[lo:hi], t0))
                f = s + int(np.searchsorted(ppos[s:hi], t1))
                p = ppos[s:f]
                assert p.size == 0 or (t0 <= p[0] and p[-1] < t1)
                acc[p] = fma32(pval[s:f].astype(np.float32), np.float32(qv[e]), acc[p])       # (distinct positions: no lost update)
        out[q] = np.float32(0) - acc
    return out


@pytest.mark.parametrize("n,nq,vocab,long_queries", CASES)
def test_twin_lists_ascend_and_terms_are_distinct(n, nq, vocab, long_queries):
    rows, _, _, _, _ = R.make_case(n, nq, vocab, long_queries)
    terms, list_off, ppos, pval = build_twin(rows)
    counts, idx, val = rows
    assert np.all(terms[1:] > terms[:-1]) and np.array_equal(terms, np.unique(idx))
    assert list_off[0] == 0 and list_off[-1] == idx.size and np.all(list_off[1:] > list_off[:-1])
    for t in range(terms.size):
        p = ppos[list_off[t]:list_off[t + 1]]
        assert np.all(p[1:] > p[:-1]), t                            # strictly: a row holds an index once
    # every posting is the stored element it came from
    ro = R.offsets(counts)
    for t in list(range(0, terms.size, max(1, terms.size // 50))):
        for j in range(list_off[t], min(list_off[t + 1], list_off[t] + 3)):
            r = int(ppos[j])
            at = np.searchsorted(idx[ro[r]:ro[r + 1]], terms[t])
            assert idx[ro[r] + at] == terms[t] and val[ro[r] + at] == pval[j]


@pytest.mark.parametrize("n,nq,vocab,long_queries", CASES)
@pytest.mark.parametrize("half", [False, True])
def test_term_at_a_time_stays_in_the_band(n, nq, vocab, long_queries, half):
    rows, queries, ref, A, m = R.make_case(n, nq, vocab, long_queries)
    if half:                    # an fp16 index: the same runs with every value rounded to half, widened exactly where read
        rows = (rows[0], rows[1], rows[2].astype(np.float16))
        queries = (queries[0], queries[1], queries[2].astype(np.float16))
        as32 = lambda b: (b[0], b[1], b[2].astype(np.float32))     # noqa: E731
        ref, A = R.sparse_reference(as32(rows), as32(queries))
    twin = build_twin(rows)
    got = term_at_a_time(twin, queries, n)
    B = (m + 1) * 2.0 ** -23 * A
    assert np.all(np.abs(got.astype(np.float64) - ref) <= B)
    assert np.all(got[m == 0] == 0.0) and not np.signbit(got[m == 0]).any()
    # lists selected from these scores pass the checker the GPU lists are held to
    for k in (1, 10, 200):
        keys, scores, counts = R.lists_from_scores(got, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


def test_tiles_give_the_same_bits_as_the_whole_range():
    n, nq = 1000, 65
    rows, queries, _, _, _ = R.make_case(n, nq, 50, False)
    twin = build_twin(rows)
    whole = term_at_a_time(twin, queries, n)
    for tile in (63, 64, 999, 1000, 1001):
        assert term_at_a_time(twin, queries, n, tile).tobytes() == whole.tobytes(), tile

"""Checker and case table for sparse search over LISTED rows (search by primary keys, batch_distance), on top of tests/sparse_ref.py,
which it imports and leaves as it is.

Query q is compared with the rows in lists[q] only, so the fp64 reference, A, m and the band B = (m + 1) * 2^-23 * A of sparse_ref
are reused unchanged and a query's answer is checked by check_sparse_lists with admissible = (row is in lists[q]) & ~excluded.
The band covers an fp32 sum of the m products in ANY order, so the order of a wave's reduction tree is covered and no tolerance of
its own is introduced here.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402


def check_by_keys(keys, scores, counts, case, lists, k, threshold, excluded, key_of_row):
    """assert that [nq][k] result lists answer "query q against the rows lists[q]".  case: sparse_ref.make_case(...); lists: per
    query the listed rows (distinct positions < n); excluded: bool [n] or None; the rest as check_sparse_lists."""
    _, _, ref, A, m = case
    nq, n = ref.shape
    assert len(lists) == nq and keys.shape == (nq, k) and scores.shape == (nq, k) and len(counts) == nq
    excluded = np.zeros(n, bool) if excluded is None else np.asarray(excluded, bool)
    for q in range(nq):
        admissible = np.zeros(n, bool)
        admissible[np.asarray(lists[q], np.int64)] = True
        admissible &= ~excluded
        R.check_sparse_lists(keys[q:q + 1], scores[q:q + 1], counts[q:q + 1], ref[q:q + 1], A[q:q + 1], m[q:q + 1], k, threshold,
                             admissible, key_of_row)


def check_batch_distance(scores, case, q, positions):
    """scores of query q of the case against `positions` in that order: within the band elementwise, exactly 0 where no index is
    shared, exactly +inf at positions >= n"""
    _, _, ref, A, m = case
    n = ref.shape[1]
    pos = np.asarray(positions, np.int64)
    scores = np.asarray(scores)
    assert scores.dtype == np.float32 and scores.shape == pos.shape
    inside = pos < n
    assert np.all(np.isposinf(scores[~inside])), "a position beyond the rows scores +inf"
    p = pos[inside]
    s = scores[inside].astype(np.float64)
    B = (m[q, p] + 1) * 2.0 ** -23 * A[q, p]
    bad = np.nonzero(np.abs(s - ref[q, p]) > B)[0]
    assert bad.size == 0, (bad[:5], s[bad[:5]], ref[q, p][bad[:5]], B[bad[:5]])
    zero = m[q, p] == 0
    assert np.all(s[zero] == 0.0) and not np.signbit(scores[inside][zero]).any(), "no shared index scores exactly +0"


def reference_lists(case, lists, k, threshold, excluded, key_of_row):
    """the answer by a plain numpy fp32 evaluation (sparse_ref.fp32_scores), restricted to the listed rows"""
    rows, queries, ref, _, _ = case
    nq, n = ref.shape
    s32 = _fp32_scores(rows, queries)
    excluded = np.zeros(n, bool) if excluded is None else np.asarray(excluded, bool)
    keys = np.full((nq, k), 0xffffffffffffffff, np.uint64)
    scores = np.zeros((nq, k), np.float32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        listed = np.zeros(n, bool)
        listed[np.asarray(lists[q], np.int64)] = True
        kq, sq, cq = R.lists_from_scores(s32[q:q + 1], k, threshold, listed & ~excluded, key_of_row)
        keys[q], scores[q], counts[q] = kq[0], sq[0], cq[0]
    return keys, scores, counts


_FP32 = {}


def _fp32_scores(rows, queries):
    key = (id(rows[0]), id(queries[0]))          # (make_case caches its arrays: one evaluation per case)
    if key not in _FP32:
        _FP32[key] = R.fp32_scores(rows, queries)
    return _FP32[key]


# ---- the list table ---------------------------------------------------------------------------------------------------------------
# sparse_ref.make_case shapes (n, nq, vocabulary, long queries) crossed with list lengths and k.  The smallest shapes that cross
# every edge of the kernel: the 64-element load boundary (rows of 64 / 65 / 4096 elements), an empty row, an empty query, a
# one-element run, the longest run (4096), a slice boundary inside a list, and a list shorter than k.
#   "edges"   query q takes length (0, 1, k - 1, k, k + 1, n)[q % 6], cut to n
#   an int    every query takes that length
#   "ragged"  every query draws its length from {0, 1, 10, 64, 500}
KS = (1, 10, 200)
TABLE = ([(65, 65, 50, False, "edges", k) for k in KS] +
         [(1000, 1, 100000, True, length, k) for length in (1, 63, 64, 65, 1000) for k in KS] +
         [(5000, 130, 50, False, "ragged", k) for k in KS])


@functools.lru_cache(maxsize=None)
def make_lists(n, nq, spec, k, seed=0):
    """per query an array of DISTINCT listed rows in random order; computed once and shared, treat as read-only"""
    rng = np.random.default_rng([seed, n, nq, k, 0 if spec == "edges" else 1 if spec == "ragged" else 2 + int(spec)])
    if spec == "edges":
        lengths = [(0, 1, k - 1, k, k + 1, n)[q % 6] for q in range(nq)]
    elif spec == "ragged":
        lengths = rng.choice([0, 1, 10, 64, 500], nq)
    else:
        lengths = [int(spec)] * nq
    out = []
    for length in lengths:
        a = rng.permutation(n)[:min(int(length), n)].astype(np.int64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)

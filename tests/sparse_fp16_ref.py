"""Cases for sparse inner-product search over fp16 values, on top of tests/sparse_ref.py (imported, left as it is).

A case of sparse_ref.make_case is rounded to half (astype(np.float16)) and its reference recomputed on the rounded values widened
back to fp32, so `rows` and `queries` of a case here are fp32 arrays whose every value is a half: casting them to float16 (which
the tests, or the Python class, do) is exact, and sparse_ref / sparse_keys_ref take the case as they take their own.

The band is unchanged.  The product of two halves has at most 22 significant bits and an exponent well inside fp32's range
(2^-48 <= |p| < 2^32), so it is exact in fp32; what is left is the fp32 sum of m exact products, which B = (m + 1) * 2^-23 * A of
sparse_ref covers in any order.

Integer cases: every value is an integer in [-8, 8] (a half), rows and queries have at most 4096 elements, so every partial sum
in any order is an integer of magnitude <= 4096 * 64 = 2^18 < 2^24: exact in fp32, and every fp32 evaluation returns the fp64
reference bit for bit.  One score is -262144, four times beyond the largest half.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402


def halves(batch):
    """(counts, indices, values) with the values as float16; exact for the cases of this module"""
    c, i, v = batch
    h = np.asarray(v).astype(np.float16)
    assert np.array_equal(h.astype(np.float32), np.asarray(v, np.float32)), "not a batch of halves"
    return c, i, h


def _rounded(batch):
    c, i, v = batch
    return c, i, np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


def _finish(rows, queries):
    ref, A = R.sparse_reference(rows, queries)
    m = R.shared_counts(rows, queries)
    for a in rows + queries + (ref, A, m):
        a.setflags(write=False)
    return rows, queries, ref, A, m


@functools.lru_cache(maxsize=None)
def make_case(n, nq, vocab, long_queries):
    """sparse_ref.make_case(...) rounded to half: (rows, queries, ref, A, m), computed once and shared; treat as read-only"""
    rows, queries = R.make_case(n, nq, vocab, long_queries)[:2]
    return _finish(_rounded(rows), _rounded(queries))


INT_N, INT_VOCAB, INT_LENGTHS = 130, 4096, (0, 1, 64, 65, 4096)


def _integer_runs(rng, lengths, full):
    counts = np.asarray(lengths, np.uint32)
    idx = [np.sort(rng.choice(INT_VOCAB, int(c), replace=False)).astype(np.uint32) for c in counts]
    val = [rng.integers(-8, 9, int(c)).astype(np.float32) for c in counts]
    for j in full:
        val[j][:] = 8.0
    return counts, np.concatenate(idx), np.concatenate(val)


@functools.lru_cache(maxsize=None)
def make_integer_case(nq):
    """130 rows of 0 / 1 / 64 / 65 / 4096 elements over a vocabulary of 4096, integer values in [-8, 8]; rows 0, 7, 129 and queries
    0, 63, 64 (those that exist) hold all 4096 indices with value 8, so their scores are -262144.  Shared, read-only."""
    rng = np.random.default_rng([16, nq])
    rl = rng.choice(INT_LENGTHS, INT_N)
    rl[:5] = INT_LENGTHS                       # every length is there
    full_rows = (0, 7, 129)
    rl[list(full_rows)] = 4096
    ql = rng.choice(INT_LENGTHS, nq)
    full_q = [q for q in (0, 63, 64) if q < nq]
    ql[full_q] = 4096
    rows = _integer_runs(rng, rl, full_rows)
    queries = _integer_runs(rng, ql, full_q)
    case = _finish(rows, queries)
    assert case[2].min() == -262144.0 and np.all(case[2] == np.round(case[2]))
    return case


def assert_exact(keys, scores, counts, ref, key_of_row):
    """every returned score equals the fp64 reference of its row bit for bit (as fp32; the reference's zeros are +0)"""
    row_of_key = {int(key_of_row[r]): r for r in range(ref.shape[1])}
    for q in range(ref.shape[0]):
        c = int(counts[q])
        want = np.array([ref[q, row_of_key[int(x)]] for x in keys[q, :c]], np.float64).astype(np.float32)
        assert np.array_equal(want.astype(np.float64), [ref[q, row_of_key[int(x)]] for x in keys[q, :c]])
        got = np.ascontiguousarray(scores[q, :c], np.float32)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (q, got, want)


def half_accumulated_scores(rows, queries):
    """the scores as an evaluation that keeps products and sums in float16 would give them (numpy, dtype=float16 throughout)"""
    rc, ri, rv = rows
    qc, qi, qv = queries
    ro, qo = R.offsets(rc), R.offsets(qc)
    out = np.zeros((len(qc), len(rc)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(len(qc)):
            dense = np.zeros(INT_VOCAB, np.float16)
            dense[qi[qo[q]:qo[q + 1]]] = np.asarray(qv[qo[q]:qo[q + 1]]).astype(np.float16)
            prod = np.asarray(rv).astype(np.float16) * dense[ri]
            for r in range(len(rc)):
                s = np.add.reduce(prod[ro[r]:ro[r + 1]], dtype=np.float16)
                out[q, r] = np.float32(0) - np.float32(s)
    return out


def sparse_lds_bytes_fp16(img_elems, k_lists):
    """sparse_lds_bytes(img_elems, k_lists, 2) of zvk_sparse.hip.h restated: lane-owned lists (64 x k scores and positions), the
    image's indices as u32, its values as halves rounded up to whole words, 16 bytes of slack"""
    return (2 * 64 * k_lists + img_elems) * 4 + ((img_elems * 2 + 3) & ~3) + 16

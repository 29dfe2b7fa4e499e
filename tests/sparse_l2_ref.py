"""fp64 reference and list checker for sparse squared-Euclidean search (numpy only), on the batches and the case table of
tests/sparse_ref.py.

A batch of sparse vectors is a triple (counts[n] uint32, indices uint32, values): the runs back to back, indices strictly
ascending inside a run.  The score of row b against query q runs over the UNION of the two index sets: a shared index adds
(b - q)^2, an index of the row alone b^2, an index of the query alone q^2.  Smaller is better, every score is >= 0.

The contract (include/zvec_hip.h, "Score, ZVEC_HIP_METRIC_L2"): s = A + R, all fp32.
  A  over the rlen stored elements of the row, any order, each step fmaf(x, x, A), x = fl(b - q) on a hit and x = b otherwise
  R  exactly +0 if hits == qlen, else max(0, Qn - Mq): Qn the fp32 sum of q^2 over the run, Mq over the matched elements

The band.  With u = 2^-24 the unit round-off:
  A   a term x^2 carries the rounding of the difference twice (it is squared) and, in a sum of rlen non-negative terms in any
      order, at most rlen roundings of partial sums (its own fmaf among them): a factor within (1 + u)^(rlen + 2) of exact, so
      |A^ - A64| <= gamma_{rlen + 2} * A64.  (An evaluation that also rounds the square before adding it has rlen + 3.)
  R   hits == qlen: exactly 0, no error.  Else Qn^ and Mq^ are sums of qlen and hits exact squares, |Qn^ - Q64| <= gamma_qlen *
      Q64 and |Mq^ - M64| <= gamma_hits * M64; the subtraction rounds once, relative to a result that is at most Q64 + M64 in
      size; the clamp at 0 moves the result towards the exact value, which is >= 0.  Together at most gamma_{qlen + 1} * (Q64 +
      M64).
  s   the final addition rounds once, relative to A^ + R^: one more unit on each of the two terms above.
2^-23 is twice the unit round-off, which covers the gamma expansion up to 4096 terms (gamma_m <= m * 2^-23 for m <= 4100), so
    B = (rlen + 4) * 2^-23 * A64  +  [hits < qlen] * (qlen + 4) * 2^-23 * (Q64 + M64).
The second term vanishes when hits == qlen, and B is 0 where the score is 0 (A64 == 0 and hits == qlen): such a pair must score
exactly +0.0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sparse_ref import CASES, lists_from_scores, make_case, offsets, random_runs  # noqa: E402,F401


def _walk(rows, queries):
    """per query: (q, row_of, b, qd, hit) over the stored elements: their values, the query's value at their index and whether the
    query has that index, all fp64 / bool"""
    rc, ri, rv = rows
    qc, qi, qv = queries
    n = len(rc)
    vocab = np.unique(np.concatenate([np.asarray(ri, np.uint32), np.asarray(qi, np.uint32)]))
    r_at = np.searchsorted(vocab, np.asarray(ri, np.uint32))
    q_at = np.searchsorted(vocab, np.asarray(qi, np.uint32))
    row_of = np.repeat(np.arange(n), np.asarray(rc, np.int64))
    qo = offsets(qc)
    b = np.asarray(rv).astype(np.float64)
    q64 = np.asarray(qv).astype(np.float64)
    for q in range(len(qc)):
        dense = np.zeros(vocab.size + 1, np.float64)
        has = np.zeros(vocab.size + 1, bool)
        dense[q_at[qo[q]:qo[q + 1]]] = q64[qo[q]:qo[q + 1]]
        has[q_at[qo[q]:qo[q + 1]]] = True
        yield q, row_of, b, dense[r_at], has[r_at]


def sparse_l2_reference(rows, queries):
    """dict of [nq][n] arrays: fp64 A64 (the exact row-side sum), Q64 (sum of q^2 of the query), M64 (sum of the matched q^2),
    score = A64 + (Q64 - M64) (the difference exactly 0 where hits == qlen), and int64 hits, rlen, qlen"""
    nq, n = len(queries[0]), len(rows[0])
    A, M = np.zeros((nq, n)), np.zeros((nq, n))
    hits = np.zeros((nq, n), np.int64)
    qo = offsets(queries[0])
    q64 = np.asarray(queries[2]).astype(np.float64)
    Q = np.array([np.sum(q64[qo[q]:qo[q + 1]] ** 2) for q in range(nq)]).reshape(nq, 1) * np.ones((1, n))
    for q, row_of, b, qd, hit in _walk(rows, queries):
        A[q] = np.bincount(row_of, weights=np.where(hit, (b - qd) ** 2, b * b), minlength=n)
        M[q] = np.bincount(row_of, weights=np.where(hit, qd * qd, 0.0), minlength=n)
        hits[q] = np.bincount(row_of, weights=hit.astype(np.float64), minlength=n).astype(np.int64)
    rlen = np.asarray(rows[0], np.int64).reshape(1, n) * np.ones((nq, 1), np.int64)
    qlen = np.asarray(queries[0], np.int64).reshape(nq, 1) * np.ones((1, n), np.int64)
    rest = np.where(hits == qlen, 0.0, np.maximum(Q - M, 0.0))
    return {"A64": A, "Q64": Q, "M64": M, "hits": hits, "rlen": rlen, "qlen": qlen, "score": A + rest}


def band(ref):
    """B of the module docstring, [nq][n]"""
    return ((ref["rlen"] + 4) * 2.0 ** -23 * ref["A64"]
            + (ref["hits"] < ref["qlen"]) * (ref["qlen"] + 4) * 2.0 ** -23 * (ref["Q64"] + ref["M64"]))


def fp32_contract_scores(rows, queries):
    """the scores by a plain numpy fp32 evaluation in the contract's structure: A, Qn and Mq each an fp32 sum in numpy's own
    order (the square rounded before it is added), then the hits == qlen rule and the clamp"""
    rc, qc = rows[0], queries[0]
    nq, n = len(qc), len(rc)
    out = np.zeros((nq, n), np.float32)
    ro = offsets(rc)[:-1]
    qo = offsets(qc)
    nonempty = np.asarray(rc) > 0
    q32 = np.asarray(queries[2]).astype(np.float32)
    zero = np.zeros(1, np.float32)
    for q, row_of, b, qd, hit in _walk(rows, queries):
        b32, qd32 = b.astype(np.float32), qd.astype(np.float32)
        x = np.where(hit, b32 - qd32, b32)
        a = np.where(nonempty, np.add.reduceat(np.concatenate([x * x, zero]), ro), np.float32(0))
        mq = np.where(nonempty, np.add.reduceat(np.concatenate([np.where(hit, qd32 * qd32, np.float32(0)), zero]), ro), np.float32(0))
        hits = np.bincount(row_of, weights=hit.astype(np.float64), minlength=n).astype(np.int64)
        run = q32[qo[q]:qo[q + 1]]
        qn = np.sum(run * run, dtype=np.float32)
        rest = np.where(hits == int(qc[q]), np.float32(0), np.maximum(np.float32(0), qn - mq))
        out[q] = (a + rest).astype(np.float32)
    return out


def check_sparse_l2_lists(keys, scores, counts, ref, k, threshold, admissible, key_of_row, exact=False):
    """assert that [nq][k] result lists are a correct answer.  ref: sparse_l2_reference; threshold: None = none; admissible: bool
    [n], False = excluded; key_of_row: [n] keys; exact: B = 0 everywhere (data whose every sum is exact in fp32).  Free: which of
    the rows whose bands overlap at the k-th place (or at the threshold) are returned, and the order of rows whose scores are
    equal.  Every returned score has its sign bit clear, and a pair with A64 == 0 and hits == qlen scores exactly +0.0."""
    s64 = ref["score"]
    nq, n = s64.shape
    B = np.zeros_like(s64) if exact else band(ref)
    zero = (ref["A64"] == 0) & (ref["hits"] == ref["qlen"])
    assert not B[zero].any()
    thr = np.inf if threshold is None else float(np.float32(threshold))
    admissible = np.asarray(admissible, bool)
    row_of_key = {int(key_of_row[r]): r for r in range(n)}
    assert len(row_of_key) == n, "the checker needs distinct keys"
    for q in range(nq):
        c = int(counts[q])
        sure = admissible & (s64[q] + B[q] <= thr)
        maybe = admissible & (s64[q] - B[q] <= thr)
        assert min(k, int(sure.sum())) <= c <= min(k, int(maybe.sum())), (q, c, int(sure.sum()), int(maybe.sum()))
        got = [int(x) for x in keys[q, :c]]
        assert len(set(got)) == c, (q, "duplicate key")
        rows = []
        for j, key in enumerate(got):
            assert key in row_of_key, (q, j, key, "unknown key")
            r = row_of_key[key]
            assert admissible[r], (q, j, key, "excluded row returned")
            s = float(scores[q, j])
            assert abs(s - s64[q, r]) <= B[q, r], (q, j, key, s, s64[q, r], B[q, r])
            assert s <= thr, (q, j, s, thr)
            assert not np.signbit(np.float32(scores[q, j])), (q, j, key, s, "a negative score or -0")
            if zero[q, r]:
                assert np.float32(scores[q, j]).tobytes() == np.float32(0.0).tobytes(), (q, j, key, s)
            rows.append(r)
        s32 = np.asarray(scores[q, :c], np.float64)
        assert np.all(s32[1:] >= s32[:-1]), (q, "not best-first")
        present = np.zeros(n, bool)
        present[rows] = True
        if c < k:
            missing = sure & ~present
        else:
            last = rows[-1]
            missing = sure & ~present & (s64[q] + B[q] + B[q, last] < s64[q, last])
        assert not missing.any(), (q, "missing strictly better rows", np.nonzero(missing)[0][:5])


_L2_CASES = {}


def make_l2_case(n, nq, vocab, long_queries, half=False):
    """(rows, queries, ref) on the rows and queries of sparse_ref.make_case, computed once and shared; read-only.  half: the
    values rounded to IEEE binary16 first (as float16 arrays), so that the reference sees what an fp16 index stores"""
    key = (n, nq, vocab, bool(long_queries), bool(half))
    if key not in _L2_CASES:
        rows, queries = make_case(n, nq, vocab, long_queries)[:2]
        if half:
            rows = (rows[0], rows[1], rows[2].astype(np.float16))
            queries = (queries[0], queries[1], queries[2].astype(np.float16))
        ref = sparse_l2_reference(rows, queries)
        for a in rows + queries + tuple(ref.values()):
            a.setflags(write=False)
        _L2_CASES[key] = (rows, queries, ref)
    return _L2_CASES[key]

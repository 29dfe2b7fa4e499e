"""fp64 reference and list checker for sparse inner-product search (numpy only), and the case table the CPU and GPU tests share.

A batch of sparse vectors is a triple (counts[n] uint32, indices uint32, values float32): the runs back to back, indices strictly
ascending inside a run.  Scores are MINUS the inner product over shared indices, smaller is better.

The band.  An fp32 sum of m products, fused or not, in any order, errs by at most gamma_{m+1} * A, A = sum |q_i * d_i| over the
shared indices.  2^-23 is twice the unit round-off, which covers the gamma expansion for m <= 4096:
    B = (m + 1) * 2^-23 * A.
"""
import functools

import numpy as np


def offsets(counts):
    o = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=o[1:])
    return o


def _terms(rows, queries):
    """per query: the stored elements' products with the query, as fp64 (exact: 24 x 24 bits), and which are shared"""
    rc, ri, rv = rows
    qc, qi, qv = queries
    n = len(rc)
    vocab = np.unique(np.concatenate([np.asarray(ri, np.uint32), np.asarray(qi, np.uint32)]))
    r_at = np.searchsorted(vocab, np.asarray(ri, np.uint32))
    q_at = np.searchsorted(vocab, np.asarray(qi, np.uint32))
    row_of = np.repeat(np.arange(n), np.asarray(rc, np.int64))
    qo = offsets(qc)
    rv64 = np.asarray(rv, np.float32).astype(np.float64)
    for q in range(len(qc)):
        dense = np.zeros(vocab.size + 1, np.float64)
        has = np.zeros(vocab.size + 1, bool)
        dense[q_at[qo[q]:qo[q + 1]]] = np.asarray(qv, np.float32)[qo[q]:qo[q + 1]].astype(np.float64)
        has[q_at[qo[q]:qo[q + 1]]] = True
        yield q, row_of, rv64 * dense[r_at], has[r_at], n


def sparse_reference(rows, queries):
    """(score, A): two [nq][n] fp64 arrays, score = -(inner product over shared indices), A = sum of the |terms|"""
    nq, n = len(queries[0]), len(rows[0])
    score, A = np.zeros((nq, n)), np.zeros((nq, n))
    for q, row_of, prod, _, _ in _terms(rows, queries):
        score[q] = -np.bincount(row_of, weights=prod, minlength=n) + 0.0
        A[q] = np.bincount(row_of, weights=np.abs(prod), minlength=n)
    return score, A


def shared_counts(rows, queries):
    """m: [nq][n] number of indices present in both row and query"""
    nq, n = len(queries[0]), len(rows[0])
    m = np.zeros((nq, n), np.int64)
    for q, row_of, _, shared, _ in _terms(rows, queries):
        m[q] = np.bincount(row_of, weights=shared.astype(np.float64), minlength=n).astype(np.int64)
    return m


def fp32_scores(rows, queries):
    """the same scores by a plain numpy fp32 evaluation: fp32 products, fp32 sums (numpy's own order)"""
    rc, ri, rv = rows
    nq, n = len(queries[0]), len(rc)
    out = np.zeros((nq, n), np.float32)
    ro = offsets(rc)
    nonempty = np.asarray(rc) > 0
    for q, _, prod, _, _ in _terms(rows, queries):
        # (the product of two fp32 numbers, rounded once to fp32; a trailing zero so that every offset is a valid start)
        p32 = np.concatenate([prod.astype(np.float32), np.zeros(1, np.float32)])
        s = np.add.reduceat(p32, ro[:-1])
        out[q] = np.where(nonempty, -s, np.float32(0)) + np.float32(0)
    return out


def check_sparse_lists(keys, scores, counts, ref, A, m, k, threshold, admissible, key_of_row):
    """assert that [nq][k] result lists are a correct answer.  ref, A, m: sparse_reference / shared_counts; threshold: None = none;
    admissible: bool [n], False = excluded; key_of_row: [n] keys.  Free: which of the rows whose bands overlap at the k-th place
    (or at the threshold) are returned, and the order of rows whose scores are equal."""
    nq, n = ref.shape
    B = (m + 1) * 2.0 ** -23 * A
    thr = np.inf if threshold is None else float(np.float32(threshold))
    admissible = np.asarray(admissible, bool)
    row_of_key = {int(key_of_row[r]): r for r in range(n)}
    assert len(row_of_key) == n, "the checker needs distinct keys"
    for q in range(nq):
        c = int(counts[q])
        sure = admissible & (ref[q] + B[q] <= thr)
        maybe = admissible & (ref[q] - B[q] <= thr)
        assert min(k, int(sure.sum())) <= c <= min(k, int(maybe.sum())), (q, c, int(sure.sum()), int(maybe.sum()))
        got = [int(x) for x in keys[q, :c]]
        assert len(set(got)) == c, (q, "duplicate key")
        rows = []
        for j, key in enumerate(got):
            assert key in row_of_key, (q, j, key, "unknown key")
            r = row_of_key[key]
            assert admissible[r], (q, j, key, "excluded row returned")
            s = float(scores[q, j])
            assert abs(s - ref[q, r]) <= B[q, r], (q, j, key, s, ref[q, r], B[q, r])
            assert s <= thr, (q, j, s, thr)
            if m[q, r] == 0:
                assert s == 0.0, (q, j, key, s)
            rows.append(r)
        s32 = np.asarray(scores[q, :c], np.float64)
        assert np.all(s32[1:] >= s32[:-1]), (q, "not best-first")
        present = np.zeros(n, bool)
        present[rows] = True
        if c < k:
            missing = sure & ~present
        else:
            last = rows[-1]
            missing = sure & ~present & (ref[q] + B[q] + B[q, last] < ref[q, last])
        assert not missing.any(), (q, "missing strictly better rows", np.nonzero(missing)[0][:5])


def lists_from_scores(s32, k, threshold, admissible, key_of_row):
    """top-k lists (keys, scores, counts) of an [nq][n] fp32 score matrix, ties in row order"""
    nq, n = s32.shape
    keys = np.full((nq, k), 0xffffffffffffffff, np.uint64)
    scores = np.zeros((nq, k), np.float32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        ok = np.asarray(admissible, bool).copy()
        if threshold is not None:
            ok &= s32[q] <= np.float32(threshold)
        cand = np.nonzero(ok)[0]
        order = cand[np.argsort(s32[q, cand], kind="stable")][:k]
        counts[q] = order.size
        keys[q, :order.size] = np.asarray(key_of_row, np.uint64)[order]
        scores[q, :order.size] = s32[q, order]
    return keys, scores, counts


# ---- the shared case table: a pairwise cover of the edges -----------------------------------------------------------------------
# (n, nq, vocabulary, k, long): k "n+5" = n + 5; long = every 7th query has 4096 elements (one-query blocks between shorter ones,
# so the batch is cut into several query blocks of unequal size).  Vocabulary 50: nearly every pair overlaps, runs of 0 / 1 / 20 /
# 50 elements.  Vocabulary 100 000: nearly none does (the all-zero tie case), rows of 0 / 1 / 64 / 65 elements and every 97th row
# 4096, queries of 0 / 1 / 40.  k 200, and n + 5 from n = 1000 on, are beyond the fused lists: the dense-score route.
CASES = [
    (1, 1, 50, 1, False), (1, 63, 100000, 10, True), (1, 130, 50, "n+5", False),
    (63, 64, 50, 10, False), (63, 1, 100000, 100, True), (63, 65, 100000, "n+5", False),
    (64, 63, 100000, 1, False), (64, 130, 50, 100, False), (64, 1, 50, 200, False),
    (65, 65, 50, 1, False), (65, 64, 100000, 10, True), (65, 63, 50, 200, False),
    (1000, 1, 50, 10, False), (1000, 130, 100000, 100, True), (1000, 64, 50, "n+5", False), (1000, 65, 100000, 1, True),
    (5000, 63, 50, 100, False), (5000, 130, 100000, 10, True), (5000, 1, 100000, "n+5", True), (5000, 65, 50, 10, False),
    (5000, 64, 100000, 200, True),
]


def random_runs(rng, lengths, vocab):
    counts = np.asarray(lengths, np.uint32)
    idx = [np.sort(rng.choice(vocab, int(c), replace=False)).astype(np.uint32) for c in counts]
    indices = np.concatenate(idx) if idx else np.zeros(0, np.uint32)
    values = rng.uniform(-1.0, 1.0, indices.size).astype(np.float32)      # mixed sign
    return counts, indices, values


@functools.lru_cache(maxsize=None)
def make_case(n, nq, vocab, long_queries, seed=0):
    """rows, queries and their reference (score, A, m), computed once and shared; treat as read-only"""
    rng = np.random.default_rng([seed, n, nq, vocab, int(long_queries)])
    if vocab >= 4096:
        rl = rng.choice([0, 1, 64, 65], n)
        rl[::97] = 4096
        ql = rng.choice([0, 1, 40], nq)
        if long_queries:
            ql[3::7] = 4096
            if nq == 1:
                ql[0] = 4096
    else:
        rl = rng.choice([0, 1, 20, vocab], n)
        ql = rng.choice([0, 1, 40], nq)
    rows = random_runs(rng, rl, vocab)
    queries = random_runs(rng, ql, vocab)
    ref, A = sparse_reference(rows, queries)
    m = shared_counts(rows, queries)
    for a in rows + queries + (ref, A, m):
        a.setflags(write=False)
    return rows, queries, ref, A, m

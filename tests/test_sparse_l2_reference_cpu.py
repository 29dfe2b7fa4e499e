"""tests/sparse_l2_ref.py checked on the CPU: the fp64 reference against a dense brute force, the band against two honest fp32
evaluations (the reference's sequential merge join, and numpy sums in the contract's A + R structure), and the checker against
wrong answers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_l2_ref as L  # noqa: E402
import sparse_ref as R  # noqa: E402


# ---- 1. the reference is the dense distance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,nq,vocab", [(1, 1, 50), (63, 64, 50), (65, 65, 50), (64, 63, 100000)])
def test_reference_equals_dense_brute_force(n, nq, vocab, half):
    rows, queries, ref = L.make_l2_case(n, nq, vocab, False, half)
    words = np.unique(np.concatenate([rows[1], queries[1]]))

    def dense(batch):
        c, i, v = batch
        o = R.offsets(c)
        out = np.zeros((len(c), words.size + 1))
        for r in range(len(c)):
            out[r, np.searchsorted(words, i[o[r]:o[r + 1]])] = v[o[r]:o[r + 1]].astype(np.float64)
        return out

    b, q = dense(rows), dense(queries)
    want = ((q[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    assert np.allclose(ref["score"], want, rtol=1e-12, atol=0)
    assert np.array_equal(ref["score"] == 0, want == 0)
    assert np.all(ref["score"] >= 0) and np.all(ref["M64"] <= ref["Q64"] * (1 + 1e-12))
    assert np.array_equal(ref["hits"], ((q[:, None, :] != 0) & (b[None, :, :] != 0)).sum(-1))      # (no stored value is 0 here)
    # where every query element met one, the rest is exactly 0 and the band has no second term
    covered = ref["hits"] == ref["qlen"]
    assert np.array_equal(ref["score"][covered], ref["A64"][covered])
    assert np.array_equal(L.band(ref)[covered], ((ref["rlen"] + 4) * 2.0 ** -23 * ref["A64"])[covered])
    assert not L.band(ref)[ref["score"] == 0].any()


# ---- 2. the reference's order of summation: a sequential fp32 merge join -----------------------------------------------------------
def merge_join_fp32(bi, bv, qi, qv):
    """both runs walked in index order, one fp32 sum: (b - q)^2 for a shared index, b^2 or q^2 for one that only one side has"""
    acc = np.float32(0)
    i = j = 0
    bv, qv = np.asarray(bv).astype(np.float32), np.asarray(qv).astype(np.float32)
    while i < len(bi) or j < len(qi):
        if j == len(qi) or (i < len(bi) and bi[i] < qi[j]):
            x = bv[i]
            i += 1
        elif i == len(bi) or qi[j] < bi[i]:
            x = qv[j]
            j += 1
        else:
            x = np.float32(bv[i] - qv[j])
            i, j = i + 1, j + 1
        acc = np.float32(acc + np.float32(x * x))
    return acc


def merge_join_fp32_small_vocab(rows, queries, vocab):
    """the same walk for every pair of a batch at once: the indices 0 .. vocab - 1 in ascending order, one fp32 addition per index
    that either side has (an index neither has adds nothing)"""
    def dense(batch):
        c, i, v = batch
        o = R.offsets(c)
        val, has = np.zeros((len(c), vocab), np.float32), np.zeros((len(c), vocab), bool)
        for r in range(len(c)):
            val[r, i[o[r]:o[r + 1]]] = v[o[r]:o[r + 1]].astype(np.float32)
            has[r, i[o[r]:o[r + 1]]] = True
        return val, has

    (b, hb), (q, hq) = dense(rows), dense(queries)
    acc = np.zeros((len(queries[0]), len(rows[0])), np.float32)
    for w in range(vocab):
        x = (b[None, :, w] - q[:, None, w]).astype(np.float32)     # (the absent side holds 0: x = b or -q exactly)
        term = (x * x).astype(np.float32)
        acc = np.where(hb[None, :, w] | hq[:, None, w], (acc + term).astype(np.float32), acc)
    return acc


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,nq,vocab,k,long_queries", [c for c in R.CASES if c[2] == 50])
def test_sequential_merge_join_stays_inside_the_band(n, nq, vocab, k, long_queries, half):
    rows, queries, ref = L.make_l2_case(n, nq, vocab, long_queries, half)
    got = merge_join_fp32_small_vocab(rows, queries, vocab)
    # (the vectorised walk is the scalar one)
    ro, qo = R.offsets(rows[0]), R.offsets(queries[0])
    for q, r in [(0, 0), (nq - 1, n - 1), (nq // 2, n // 3)]:
        one = merge_join_fp32(rows[1][ro[r]:ro[r + 1]], rows[2][ro[r]:ro[r + 1]], queries[1][qo[q]:qo[q + 1]], queries[2][qo[q]:qo[q + 1]])
        assert one.tobytes() == got[q, r].tobytes()
    err = np.abs(got.astype(np.float64) - ref["score"])
    assert np.all(err <= L.band(ref)), float((err - L.band(ref)).max())


@pytest.mark.parametrize("half", [False, True])
def test_sequential_merge_join_of_one_longest_pair(half):
    rng = np.random.default_rng(21)
    rows = R.random_runs(rng, [4096], 6000)
    queries = R.random_runs(rng, [4096], 6000)
    if half:
        rows, queries = [(c, i, v.astype(np.float16)) for c, i, v in (rows, queries)]
    ref = L.sparse_l2_reference(rows, queries)
    assert 2000 < ref["hits"][0, 0] < 4096
    got = merge_join_fp32(rows[1], rows[2], queries[1], queries[2])
    assert abs(float(got) - ref["score"][0, 0]) <= L.band(ref)[0, 0]


# ---- 3. the band is not too tight for an honest implementation ---------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,nq,vocab,k,long_queries", R.CASES)
def test_fp32_evaluation_in_the_contracts_structure_stays_inside_the_band(n, nq, vocab, k, long_queries, half):
    rows, queries, ref = L.make_l2_case(n, nq, vocab, long_queries, half)
    got = L.fp32_contract_scores(rows, queries)
    B = L.band(ref)
    err = np.abs(got.astype(np.float64) - ref["score"])
    assert np.all(err <= B), float((err - B).max())
    assert not np.signbit(got).any()
    zero = (ref["A64"] == 0) & (ref["hits"] == ref["qlen"])
    assert not got[zero].any()
    k = n + 5 if k == "n+5" else k
    key_of_row = np.arange(n, dtype=np.uint64) * np.uint64(5) + np.uint64(1)
    keys, scores, counts = R.lists_from_scores(got, k, None, np.ones(n, bool), key_of_row)
    L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, np.ones(n, bool), key_of_row)


# ---- 4. the checker rejects wrong answers --------------------------------------------------------------------------------------------
def _self_case(half=False):
    rng = np.random.default_rng(22)
    rows = R.random_runs(rng, [1, 20, 64, 65, 300, 40, 7, 4096], 5000)
    if half:
        rows = (rows[0], rows[1], rows[2].astype(np.float16))
    return rows, L.sparse_l2_reference(rows, rows)


def _norm_expansion_scores(rows, queries):
    """|b|^2 + |q|^2 - 2 b.q in fp32: what the contract refuses"""
    ro, qo = R.offsets(rows[0]), R.offsets(queries[0])
    v32, q32 = rows[2].astype(np.float32), queries[2].astype(np.float32)
    bn = np.array([np.sum(v32[ro[r]:ro[r + 1]] ** 2, dtype=np.float32) for r in range(len(rows[0]))], np.float32)
    qn = np.array([np.sum(q32[qo[q]:qo[q + 1]] ** 2, dtype=np.float32) for q in range(len(queries[0]))], np.float32)
    dot = -R.fp32_scores((rows[0], rows[1], v32), (queries[0], queries[1], q32))
    return ((bn[None, :] + qn[:, None]).astype(np.float32) - np.float32(2) * dot).astype(np.float32)


def test_checker_rejects_the_norm_expansion_on_a_self_query():
    rows, ref = _self_case()
    n = len(rows[0])
    assert not np.diag(ref["score"]).any() and not np.diag(L.band(ref)).any()
    key_of_row = np.arange(n, dtype=np.uint64)
    good = L.fp32_contract_scores(rows, rows)
    assert not np.diag(good).any()
    L.check_sparse_l2_lists(*R.lists_from_scores(good, 3, None, np.ones(n, bool), key_of_row), ref, 3, None, np.ones(n, bool), key_of_row)
    bad = _norm_expansion_scores(rows, rows)
    assert np.diag(bad).any(), "the expansion happens to cancel exactly: pick other data"
    with pytest.raises(AssertionError):
        L.check_sparse_l2_lists(*R.lists_from_scores(bad, 3, None, np.ones(n, bool), key_of_row), ref, 3, None, np.ones(n, bool),
                                key_of_row)


def test_checker_rejects_a_moved_score_an_excluded_row_and_a_missing_row():
    n, nq, k = 1000, 64, 10
    rows, queries, ref = L.make_l2_case(n, nq, 50, False)
    B = L.band(ref)
    key_of_row = np.arange(n, dtype=np.uint64)
    good = L.fp32_contract_scores(rows, queries)
    admissible = np.ones(n, bool)
    keys, scores, counts = R.lists_from_scores(good, k, None, admissible, key_of_row)
    L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, admissible, key_of_row)
    # one score moved by twice its band (the list stays ascending: the last entry moves up)
    q = int(np.nonzero(queries[0] == 40)[0][0])            # (a query that holds something: no row is at distance 0 of it)
    assert counts[q] == k
    r = int(keys[q, k - 1])
    assert B[q, r] > 0
    moved = scores.copy()
    moved[q, k - 1] = np.float32(ref["score"][q, r] + 2 * B[q, r])
    assert abs(float(moved[q, k - 1]) - ref["score"][q, r]) > B[q, r]
    with pytest.raises(AssertionError):
        L.check_sparse_l2_lists(keys, moved, counts, ref, k, None, admissible, key_of_row)
    # an excluded row in a list
    banned = admissible.copy()
    banned[int(keys[q, 0])] = False
    with pytest.raises(AssertionError):
        L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, banned, key_of_row)
    # a strictly better row left out: the best one, the list shifted up and refilled from rank k + 1
    order = np.argsort(ref["score"][q], kind="stable")
    assert ref["score"][q, order[0]] + B[q, order[0]] + B[q, order[k]] < ref["score"][q, order[k]]
    k1, s1, c1 = R.lists_from_scores(good, k + 1, None, admissible, key_of_row)
    without = (keys.copy(), scores.copy(), counts)
    without[0][q], without[1][q] = k1[q, 1:], s1[q, 1:]
    assert int(order[0]) not in without[0][q].tolist()
    with pytest.raises(AssertionError):
        L.check_sparse_l2_lists(*without, ref, k, None, admissible, key_of_row)
    # exact = True leaves no band at all: the honest fp32 scores of real-valued data are refused
    with pytest.raises(AssertionError):
        L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, admissible, key_of_row, exact=True)

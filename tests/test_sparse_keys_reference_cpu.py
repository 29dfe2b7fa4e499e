"""The checker for sparse search over listed rows (tests/sparse_keys_ref.py) on the CPU: a plain fp32 evaluation restricted to the
listed rows passes it on every entry of the table, seeded mutations of a correct answer each fail it, and the two entry points
are declared and exported."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_keys_ref as K  # noqa: E402
import sparse_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zvec_hip_sparse_search_by_ids", "zvec_hip_sparse_batch_distance")


@pytest.mark.parametrize("n,nq,vocab,long_queries,spec,k", K.TABLE)
def test_fp32_evaluation_of_the_listed_rows_passes(n, nq, vocab, long_queries, spec, k):
    case = R.make_case(n, nq, vocab, long_queries)
    lists = K.make_lists(n, nq, spec, k)
    key_of_row = np.arange(n, dtype=np.uint64)
    keys, scores, counts = K.reference_lists(case, lists, k, None, None, key_of_row)
    assert counts.tolist() == [min(k, len(a)) for a in lists]
    K.check_by_keys(keys, scores, counts, case, lists, k, None, None, key_of_row)


@pytest.mark.parametrize("thr", [-0.75, 0.0, 0.3])
def test_fp32_evaluation_passes_with_threshold_and_exclusions(thr):
    n, nq, k = 5000, 130, 10
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", k)
    key_of_row = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1 << 40)
    excluded = np.random.default_rng(11).random(n) < 0.3
    keys, scores, counts = K.reference_lists(case, lists, k, thr, excluded, key_of_row)
    K.check_by_keys(keys, scores, counts, case, lists, k, thr, excluded, key_of_row)


def test_batch_distance_checker():
    n = 1000
    case = R.make_case(n, 1, 100000, True)
    rows, queries, ref, A, m = case
    s32 = R.fp32_scores(rows, queries)
    pos = np.concatenate([np.random.default_rng(2).permutation(n)[:300], [5, 5, n, n + 7, 0xffffffff]]).astype(np.int64)
    out = np.where(pos < n, s32[0, np.minimum(pos, n - 1)], np.float32(np.inf)).astype(np.float32)
    K.check_batch_distance(out, case, 0, pos)
    shared = np.nonzero((pos < n) & (m[0, np.minimum(pos, n - 1)] > 0))[0]
    assert shared.size
    bad = out.copy()
    j = int(shared[0])
    bad[j] += np.float32(2 * (m[0, pos[j]] + 1) * 2.0 ** -23 * A[0, pos[j]] + 1e-6)
    with pytest.raises(AssertionError):
        K.check_batch_distance(bad, case, 0, pos)
    bad = out.copy()
    bad[-1] = 0.0
    with pytest.raises(AssertionError):
        K.check_batch_distance(bad, case, 0, pos)


# ---- mutations: each must FAIL the checker --------------------------------------------------------------------------------------
def _setup(k=10):
    n, nq = 5000, 130
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", k)
    key_of_row = np.arange(n, dtype=np.uint64)
    keys, scores, counts = K.reference_lists(case, lists, k, None, None, key_of_row)
    K.check_by_keys(keys, scores, counts, case, lists, k, None, None, key_of_row)
    return n, case, lists, key_of_row, keys.copy(), scores.copy(), counts.copy()


def _fails(keys, scores, counts, case, lists, k, excluded, key_of_row):
    with pytest.raises(AssertionError):
        K.check_by_keys(keys, scores, counts, case, lists, k, None, excluded, key_of_row)


def _a_query(lists, counts, at_least):
    return next(q for q in range(len(lists)) if len(lists[q]) >= at_least and counts[q] >= min(at_least, 10))


def test_mutation_best_listed_row_replaced_by_an_unlisted_row():
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    q = _a_query(lists, counts, 10)
    unlisted = next(r for r in range(n) if r not in set(lists[q].tolist()))
    keys[q, 0] = key_of_row[unlisted]
    _fails(keys, scores, counts, case, lists, k, None, key_of_row)


def test_mutation_excluded_row_returned():
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    q = _a_query(lists, counts, 64)
    excluded = np.zeros(n, bool)
    excluded[int(keys[q, 0])] = True            # (key == position here)
    _fails(keys, scores, counts, case, lists, k, excluded, key_of_row)


def test_mutation_score_moved_out_of_the_band():
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    _, _, ref, A, m = case
    q = _a_query(lists, counts, 64)
    j = int(counts[q]) - 1                        # (the last entry, moved up: the list stays best-first)
    r = int(keys[q, j])
    scores[q, j] += np.float32(2 * (m[q, r] + 1) * 2.0 ** -23 * A[q, r] + 1e-6)
    _fails(keys, scores, counts, case, lists, k, None, key_of_row)


def test_mutation_strictly_better_listed_row_dropped():
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    _, _, ref, A, m = case
    B = (m + 1) * 2.0 ** -23 * A
    done = 0
    for q in range(len(lists)):
        if len(lists[q]) < 64:
            continue
        # the answer without the best row: the next best listed row takes the free place
        best = int(keys[q, 0])
        rest = np.asarray([r for r in lists[q] if r != best], np.int64)
        sub = [rest if i == q else lists[i] for i in range(len(lists))]
        k2, s2, c2 = K.reference_lists(case, sub, k, None, None, key_of_row)
        last = int(k2[q, k - 1])
        if not ref[q, best] + B[q, best] + B[q, last] < ref[q, last]:
            continue                              # (not STRICTLY better than the new last entry: the checker leaves that free)
        keys[q], scores[q], counts[q] = k2[q], s2[q], c2[q]
        done += 1
        break
    assert done == 1
    _fails(keys, scores, counts, case, lists, k, None, key_of_row)


@pytest.mark.parametrize("delta", [-1, 1])
def test_mutation_counts_off_by_one(delta):
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    q = next(q for q in range(len(lists)) if len(lists[q]) == 1) if delta > 0 else _a_query(lists, counts, 10)
    counts[q] = int(counts[q]) + delta
    _fails(keys, scores, counts, case, lists, k, None, key_of_row)


def test_mutation_lists_not_best_first():
    k = 10
    n, case, lists, key_of_row, keys, scores, counts = _setup(k)
    q = next(q for q in range(len(lists)) if counts[q] == k and scores[q, 0] < scores[q, k - 1])
    keys[q, [0, k - 1]] = keys[q, [k - 1, 0]]
    scores[q, [0, k - 1]] = scores[q, [k - 1, 0]]
    _fails(keys, scores, counts, case, lists, k, None, key_of_row)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    so = os.path.join(ROOT, "zvec_amd", "libzvec_hip.so")
    if not os.path.exists(so):
        pytest.skip("libzvec_hip.so not built")
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(zvec_hip_[a-z_0-9]+)\s*\(", text))
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", so]).decode().splitlines() if line.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
    from zvec_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name

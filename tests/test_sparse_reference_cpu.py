"""The sparse inner-product reference and its list checker (tests/sparse_ref.py) on hand-computed cases, the checker's refusals,
and the checker against a plain numpy fp32 evaluation of every shape the GPU test uses: the reference passes its own checker
before the GPU is asked to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(vectors):
    counts = np.array([len(v) for v in vectors], np.uint32)
    idx = np.array([i for v in vectors for i, _ in v], np.uint32)
    val = np.array([x for v in vectors for _, x in v], np.float32)
    return counts, idx, val


ROWS = _batch([[(1, 2.0), (5, -1.0), (9, 0.5)], [], [(5, 4.0)], [(2, 1.0), (3, 1.0)], [(1, -3.0), (9, 2.0)]])
QUERIES = _batch([[(1, 1.0), (9, 2.0)], [], [(5, -2.0), (7, 1.0)]])


def test_reference_on_hand_computed_rows():
    score, A = R.sparse_reference(ROWS, QUERIES)
    m = R.shared_counts(ROWS, QUERIES)
    assert score.tolist() == [[-3.0, 0.0, 0.0, 0.0, -1.0], [0.0] * 5, [-2.0, 0.0, 8.0, 0.0, 0.0]]
    assert A.tolist() == [[3.0, 0.0, 0.0, 0.0, 7.0], [0.0] * 5, [2.0, 0.0, 8.0, 0.0, 0.0]]
    assert m.tolist() == [[2, 0, 0, 0, 2], [0] * 5, [1, 0, 1, 0, 0]]
    assert not np.signbit(score).any() or (score[np.signbit(score)] < 0).all()       # zeros are +0
    assert R.fp32_scores(ROWS, QUERIES).tolist() == score.tolist()


def _good(k=3, threshold=None, admissible=None):
    score, A = R.sparse_reference(ROWS, QUERIES)
    m = R.shared_counts(ROWS, QUERIES)
    adm = np.ones(5, bool) if admissible is None else admissible
    key_of_row = np.arange(100, 105, dtype=np.uint64)
    lists = R.lists_from_scores(R.fp32_scores(ROWS, QUERIES), k, threshold, adm, key_of_row)
    return lists, (score, A, m, k, threshold, adm, key_of_row)


def test_checker_accepts_correct_lists():
    for k in (1, 3, 5, 8):
        (keys, scores, counts), rest = _good(k)
        R.check_sparse_lists(keys, scores, counts, *rest)
    (keys, scores, counts), rest = _good(5, threshold=-0.5)
    assert counts.tolist() == [2, 0, 1]
    R.check_sparse_lists(keys, scores, counts, *rest)
    (keys, scores, counts), rest = _good(5, admissible=np.array([0, 1, 1, 1, 1], bool))
    R.check_sparse_lists(keys, scores, counts, *rest)
    # equal scores may come in any order, and any of them may sit at the k-th place
    (keys, scores, counts), rest = _good(2)
    keys[1] = [104, 102]
    R.check_sparse_lists(keys, scores, counts, *rest)


def test_checker_rejects_wrong_lists():
    def refused(mutate, **kw):
        (keys, scores, counts), rest = _good(**kw)
        mutate(keys, scores, counts)
        with pytest.raises(AssertionError):
            R.check_sparse_lists(keys, scores, counts, *rest)

    def wrong_score(keys, scores, counts):
        scores[0, 0] = np.nextafter(np.float32(-3.0), np.float32(0), dtype=np.float32) + np.float32(1e-5)

    def missing_better(keys, scores, counts):      # query 0: row 4 (-1) dropped for a zero row
        keys[0, 1], scores[0, 1] = 101, 0.0
        keys[0, 2] = 102

    def duplicate(keys, scores, counts):
        keys[0, 2] = keys[0, 1]
        scores[0, 2] = scores[0, 1]

    def short_count(keys, scores, counts):
        counts[2] = 2

    def unordered(keys, scores, counts):
        keys[0, 0], keys[0, 1] = keys[0, 1], keys[0, 0]
        scores[0, 0], scores[0, 1] = scores[0, 1], scores[0, 0]

    def nonzero_without_overlap(keys, scores, counts):
        scores[1, 0] = np.float32(1e-30)

    for f in (wrong_score, missing_better, duplicate, short_count, unordered, nonzero_without_overlap):
        refused(f)
    # an excluded row in a list
    (keys, scores, counts), rest = _good(3)
    rest = rest[:5] + (np.array([0, 1, 1, 1, 1], bool),) + rest[6:]
    with pytest.raises(AssertionError):
        R.check_sparse_lists(keys, scores, counts, *rest)
    # a row beyond the threshold
    (keys, scores, counts), rest = _good(3)
    rest = rest[:4] + (-0.5,) + rest[5:]
    with pytest.raises(AssertionError):
        R.check_sparse_lists(keys, scores, counts, *rest)


@pytest.mark.parametrize("n,nq,vocab,k,long_queries", R.CASES)
def test_checker_accepts_numpy_fp32_on_the_gpu_cases(n, nq, vocab, k, long_queries):
    rows, queries, ref, A, m = R.make_case(n, nq, vocab, long_queries)
    assert rows[0].max() <= 4096 and (vocab < 4096 or n < 1 or rows[0][0] == 4096)
    k = n + 5 if k == "n+5" else k
    key_of_row = np.arange(n, dtype=np.uint64)
    adm = np.ones(n, bool)
    keys, scores, counts = R.lists_from_scores(R.fp32_scores(rows, queries), k, None, adm, key_of_row)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, adm, key_of_row)


def test_header_declares_the_sparse_entries_and_binding_agrees():
    from zvec_amd import _lib
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    for name in ("create", "destroy", "reserve", "append", "count", "get_vector", "search", "search_dev"):
        assert "zvec_hip_sparse_%s(" % name in text
        assert "zvec_hip_sparse_" + name in _lib.SYMBOLS
    assert "#define ZVEC_HIP_ABI_VERSION 1" in text


def test_c_example_compiles_as_c99():
    import subprocess
    import tempfile
    from zvec_amd import _lib
    _lib.library_path()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sparse_search")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "sparse_search.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-lm",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        assert os.path.exists(exe)

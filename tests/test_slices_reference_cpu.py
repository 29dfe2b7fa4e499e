"""The preconditions of the query-slicing fixtures (tests/slices_ref.py), held on the CPU: a fixture that silently stops slicing,
or whose answers on the two sides of a slice boundary could be mistaken for one another, fails here instead of passing
tests/test_gpu_query_slices.py."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slices_ref as S  # noqa: E402

NAMES = list(S.FIXTURES)


def test_restated_sub_batch():
    assert S.dense_sub_batch(300, 1) == 300                       # the cap
    assert S.dense_sub_batch(300, 2 ** 28) == 1 and S.dense_sub_batch(300, 2 ** 29) == 1          # exactly 1 GiB; never 0
    assert S.dense_sub_batch(300, 2 ** 20) == 256 and S.dense_sub_batch(300, 2 ** 20 + 1) == 255


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_slices(name):
    fx = S.FIXTURES[name]
    w, count = S.slice_width(fx), fx["count"]
    nslices = (count + w - 1) // w
    assert nslices >= 2 and len(S.boundaries(fx)) == nslices - 1
    if name in S.GIB_FIXTURES:
        assert count * S.row_floats(fx) * 4 > S.GIB              # the cap itself cuts the batch, not the 32768 limit
        assert count <= 32768
    else:
        assert count > 32768 and w == 32768


@pytest.mark.parametrize("name", NAMES)
def test_checked_queries_cover_slices_and_boundaries(name):
    fx = S.FIXTURES[name]
    sel = S.checked_queries(fx)
    assert sel == sorted(set(sel)) and 0 <= sel[0] and sel[-1] == fx["count"] - 1 and sel[0] == 0
    assert {S.slice_of(fx, q) for q in sel} == set(range(len(S.boundaries(fx)) + 1))
    for b in S.boundaries(fx):
        assert b - 1 in sel and b in sel
        assert S.slice_of(fx, b - 1) + 1 == S.slice_of(fx, b)
    assert len(sel) <= 2 + 2 * S.NEAR * len(S.boundaries(fx))    # (a reference for these only)


def test_widths_straddle_the_kernels_blocks():
    """a slice boundary falls inside a 64-query sparse plan block, a 32-query Hamming block and a 128-query scan tile of the
    uncut batch: only a loop that cuts there gets it right.  (The 32768 of the other two fixtures is the code's own figure.)"""
    for name in S.GIB_FIXTURES:
        fx = S.FIXTURES[name]
        block = {1: S.WIDE_ROWS, 2: S.HAM_QB}.get(fx["loop"], S.SPARSE_QB)
        assert S.slice_width(fx) % block != 0, name
    # the three sparse loops over the large index share rows, queries and reference: same widths, same checked queries
    assert len({tuple(S.checked_queries(S.FIXTURES[n])) for n in S.GIB_FIXTURES if S.FIXTURES[n]["loop"] >= 3}) == 1


def test_k_is_beyond_the_fused_lists():
    kmax = S.flat_fused_max_k()
    lds = lambda k: (2 * 32 * 32 + 2 * 128 * 32 + 7 * 32 + 4 + 2 * 32 * k) * 4          # scan_lds_bytes(1, k)
    assert lds(kmax) <= 160 * 1024 - 1024 < lds(kmax + 1)
    assert S.FIXTURES["flat_large_k"]["k"] > kmax
    assert S.FIXTURES["flat_large_k"]["k"] * 12 + 16 <= 60 * 1024               # (and the merge list still fits: merge_fits)
    assert S.FIXTURES["hamming"]["k"] > S.HAM_FUSED_MAX_K
    assert S.FIXTURES["sparse_scan"]["k"] > S.SPARSE_FUSED_MAX_K


def test_every_query_differs():
    assert S.all_differ(S.dense_data()[1])
    assert S.all_differ(S.hamming_data()[1])
    for count in sorted({S.FIXTURES[n]["count"] for n in S.SPARSE_FIXTURES}):
        q = S.sparse_queries(count)
        assert S.sparse_queries_differ(q)
        assert q[0].min() >= 3 and q[0].max() <= 8 and len(set(q[0][:16].tolist())) > 2          # varying lengths
    for n in sorted({S.FIXTURES[n]["n"] for n in S.SPARSE_FIXTURES}):
        c, i, v = S.sparse_rows(n)
        o = S.R.offsets(c)
        assert c.min() >= 1 and c.max() == 4 and 3.5 < c.mean() <= 4
        inner = np.ones(i.size, bool)
        inner[o[:-1]] = False
        assert np.all(i[inner] > i[np.nonzero(inner)[0] - 1]) and i.max() < S.VOCAB and np.all(v != 0)
    lists = S.id_lists()
    assert min(len(a) for a in lists) == 1 and max(len(a) for a in lists) == 4


def _opposite_pairs(fx):
    sel = S.checked_queries(fx)
    return [(a, b) for a, b in itertools.combinations(range(len(sel)), 2) if S.slice_of(fx, sel[a]) != S.slice_of(fx, sel[b])]


def _assert_sets_differ(fx, key_sets, what):
    sel = S.checked_queries(fx)
    for a, b in _opposite_pairs(fx):
        assert key_sets[a] != key_sets[b], "%s: queries %d and %d, in different slices, have the same reference answer" % (what, sel[a], sel[b])


@pytest.mark.parametrize("metric", S.FIXTURES["flat_large_k"]["metrics"])
def test_flat_answers_differ_across_boundaries(metric):
    fx = S.FIXTURES["flat_large_k"]
    ref = S.dense_reference(metric)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)          # exact in fp32
    pos, _, cnt = S.top_lists(ref, fx["k"])
    assert np.all(cnt == fx["k"])
    _assert_sets_differ(fx, [frozenset(p.tolist()) for p in pos], metric)
    # ... and among the rows the exclusion bitset leaves: more than half of them, or the search would compact the kept rows
    # and the narrower score matrix would no longer be sliced
    keep = ~S.exclude_mask(fx["n"])
    assert 0.5 * fx["n"] < keep.sum() < 0.6 * fx["n"]
    pos, _, cnt = S.top_lists(ref, fx["k"], keep)
    assert np.all(cnt == fx["k"])
    _assert_sets_differ(fx, [frozenset(p.tolist()) for p in pos], metric + " with exclusion")


def test_a_norm_that_is_not_offset_changes_the_l2_answer():
    """the planted pair of dense_data: scored with query 0's norm, the first query of the second slice has most rows clamped
    to 0, and the re-scored selection is not the k nearest: check_exact_list refuses it.  (The other checked queries of that
    slice carry random norms on both sides; whether the mutant shows there is left open.)"""
    fx = S.FIXTURES["flat_large_k"]
    sel, k, key_of = S.checked_queries(fx), fx["k"], S.sparse_key_of(fx["n"])
    q = S.dense_data()[1]
    w = S.slice_width(fx)
    qn = (q.astype(np.float64) ** 2).sum(1)
    assert qn[0] == 5 and qn[w] == 36 * fx["dim"] and w in sel
    ref = S.dense_reference("SquaredEuclidean")
    mutant = S.norm_mutant_lists()
    assert sorted(mutant) == [qi for qi in sel if qi >= w]
    pos, dist = mutant[w]
    j = sel.index(w)
    want = np.sort(ref[j])[:k]
    assert int((ref[j] <= qn[w] - qn[0]).sum()) > 100 * k                   # rows that clamp to 0 and tie
    assert dist[-1] > want[-1] and (dist != want).sum() > k // 2
    with pytest.raises(AssertionError, match="scores differ"):
        S.check_exact_list(key_of[pos], dist.astype(np.float32), k, ref[j], k, key_of)


def test_hamming_answers_differ_across_boundaries():
    fx = S.FIXTURES["hamming"]
    pos, _, cnt = S.top_lists(S.hamming_scores().astype(np.float64), fx["k"])
    assert np.all(cnt == fx["k"])
    _assert_sets_differ(fx, [frozenset(p.tolist()) for p in pos], "hamming")


@pytest.mark.parametrize("name", ["sparse_scan", "sparse_inverted"])
def test_sparse_answers_differ_across_boundaries(name):
    fx = S.FIXTURES[name]
    ref = S.sparse_case(name)[2]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)          # integers: exact in fp32
    pos, _, cnt = S.top_lists(ref, fx["k"])
    assert np.all(cnt == fx["k"])
    _assert_sets_differ(fx, [frozenset(p.tolist()) for p in pos], name)


def test_the_list_checker_refuses_the_other_slices_answer():
    """check_exact_list on the reference's own lists: a query's list passes, the list of the query across the boundary (what a
    dropped q0 would return) does not, nor does a list whose scores belong to other rows"""
    fx = S.FIXTURES["sparse_scan"]
    sel, k, key_of = S.checked_queries(fx), fx["k"], S.sparse_key_of(fx["n"])
    ref = S.sparse_case("sparse_scan")[2]
    pos, scores, cnt = S.top_lists(ref, k)
    keys = key_of[pos.astype(np.int64)]
    b = S.boundaries(fx)[0]
    lo, hi = sel.index(b - 1), sel.index(b)
    for j in (lo, hi):
        S.check_exact_list(keys[j], scores[j], cnt[j], ref[j], k, key_of, what=S.where(fx, sel[j]))
    with pytest.raises(AssertionError):
        S.check_exact_list(keys[lo], scores[lo], cnt[lo], ref[hi], k, key_of)
    with pytest.raises(AssertionError, match="their own scores"):
        S.check_exact_list(keys[lo], scores[hi], cnt[hi], ref[hi], k, key_of)
    with pytest.raises(AssertionError):                       # (its best row excluded)
        S.check_exact_list(keys[hi], scores[hi], cnt[hi], ref[hi], k, key_of, admissible=np.arange(fx["n"]) != int(pos[hi][0]))


@pytest.mark.parametrize("name", ["sparse_group_gib", "sparse_group_32768", "sparse_group_ids_32768"])
def test_grouped_answers_differ_across_boundaries(name):
    fx = S.FIXTURES[name]
    groups, ngroups, keys, scores, counts = S.group_want(name)
    assert ngroups.max() >= 1
    answers = [(groups[j].tobytes(), keys[j].tobytes(), counts[j].tobytes()) for j in range(len(ngroups))]
    _assert_sets_differ(fx, answers, name)

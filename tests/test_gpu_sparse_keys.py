"""Sparse rows searched by primary keys on the GPU (zvec_hip_sparse_search_by_ids, zvec_hip_sparse_batch_distance) against
tests/sparse_keys_ref.py: query q meets the rows of its own list only, and every list is checked against the fp64 reference within
the band B = (m + 1) * 2^-23 * A of tests/sparse_ref.py (which covers the order of the wave's reduction tree)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_keys_ref as K  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -12, -31


def _key_of_row(n, given):
    return np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(1 << 40) if given else np.arange(n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _index(n, nq, vocab, long_queries, keys_given=False):
    """one index per case, shared (nothing below changes it); keys given: key = position * 7 + 2^40, appended in unequal pieces"""
    import zvec_amd as zv
    rows = R.make_case(n, nq, vocab, long_queries)[0]
    se = zv.HipFlatSparseStreamer()
    counts, idx, val = rows
    off = R.offsets(counts)
    keys = _key_of_row(n, True) if keys_given else None
    cuts = sorted({0, min(1, n), min(64, n), min(129, n), (n * 7) // 10, n}) if keys_given else [0, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], None if keys is None else keys[a:b]) == 0
    assert se.count() == n
    return se


def _search(se, queries, p_keys, k, threshold=None, exclude=None, filter_fn=None):
    ctx = se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    if filter_fn is not None:
        ctx.set_filter(filter_fn)
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys, len(queries[0]), ctx) == 0
    assert ctx.keys.shape == (len(queries[0]), k)
    return ctx.keys, ctx.scores, ctx.counts


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _p_keys(lists, key_of_row):
    return [key_of_row[a] for a in lists]


@pytest.mark.parametrize("keys_given", [False, True])
@pytest.mark.parametrize("n,nq,vocab,long_queries,spec,k", K.TABLE)
def test_table_against_the_reference(n, nq, vocab, long_queries, spec, k, keys_given):
    case = R.make_case(n, nq, vocab, long_queries)
    lists = K.make_lists(n, nq, spec, k)
    key_of_row = _key_of_row(n, keys_given)
    se = _index(n, nq, vocab, long_queries, keys_given)
    keys, scores, counts = _search(se, case[1], _p_keys(lists, key_of_row), k)
    assert counts.tolist() == [min(k, len(a)) for a in lists]
    K.check_by_keys(keys, scores, counts, case, lists, k, None, None, key_of_row)


def test_unknown_keys_are_dropped():
    n, nq, k = 5000, 130, 10
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", k)
    key_of_row = _key_of_row(n, True)
    se = _index(n, nq, 50, False, True)
    rng = np.random.default_rng(3)
    unknown = np.array([0, 5, n, (1 << 40) + 1, (1 << 40) + 7 * n, 0xfffffffffffffffe], np.uint64)     # (no multiple of 7 above 2^40 below n)
    mixed = []
    for a in lists:
        ks = key_of_row[a].tolist()
        for u in rng.choice(unknown, rng.integers(0, 4)):
            ks.insert(int(rng.integers(0, len(ks) + 1)), int(u))
        mixed.append(np.asarray(ks, np.uint64))
    keys, scores, counts = _search(se, case[1], mixed, k)
    K.check_by_keys(keys, scores, counts, case, lists, k, None, None, key_of_row)
    plain = _search(se, case[1], _p_keys(lists, key_of_row), k)
    assert counts.tolist() == plain[2].tolist() and scores.tobytes() == plain[1].tobytes()


@pytest.mark.parametrize("k", [10, 200])
def test_exclude_bitset(k):
    n, nq = 5000, 130
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", 10)
    key_of_row = _key_of_row(n, False)
    se = _index(n, nq, 50, False)
    p_keys = _p_keys(lists, key_of_row)
    listed = np.zeros(n, bool)
    for a in lists:
        listed[a] = True
    long_q = [q for q in range(nq) if len(lists[q]) == 500]
    assert long_q
    # bits on listed rows: a random half of them, and the first 128 entries of a long list (whole slices of it, whatever their length)
    mask = (np.random.default_rng(5).random(n) < 0.5) & listed
    mask[lists[long_q[0]][:128]] = True
    keys, scores, counts = _search(se, case[1], p_keys, k, exclude=_words_of(mask))
    K.check_by_keys(keys, scores, counts, case, lists, k, None, mask, key_of_row)
    # every listed row
    keys, scores, counts = _search(se, case[1], p_keys, k, exclude=_words_of(listed))
    assert not counts.any()
    # bits on unlisted rows only: no effect
    plain = _search(se, case[1], p_keys, k)
    keys, scores, counts = _search(se, case[1], p_keys, k, exclude=_words_of(~listed))
    K.check_by_keys(keys, scores, counts, case, lists, k, None, ~listed, key_of_row)
    assert counts.tolist() == plain[2].tolist() and scores.tobytes() == plain[1].tobytes() and keys.tobytes() == plain[0].tobytes()


def test_filter_callback_is_equivalent_to_the_bitset():
    n, nq, k = 5000, 130, 10
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", k)
    key_of_row = _key_of_row(n, True)
    se = _index(n, nq, 50, False, True)
    p_keys = _p_keys(lists, key_of_row)
    mask = np.random.default_rng(6).random(n) < 0.4
    row_of_key = {int(key_of_row[r]): r for r in range(n)}
    by_filter = _search(se, case[1], p_keys, k, filter_fn=lambda key: bool(mask[row_of_key[key]]))
    by_bits = _search(se, case[1], p_keys, k, exclude=_words_of(mask))
    for keys, scores, counts in (by_filter, by_bits):
        K.check_by_keys(keys, scores, counts, case, lists, k, None, mask, key_of_row)
    assert by_filter[2].tolist() == by_bits[2].tolist() and by_filter[1].tobytes() == by_bits[1].tobytes()


@pytest.mark.parametrize("k", [10, 200])
def test_threshold(k):
    n, nq = 5000, 130
    case = R.make_case(n, nq, 50, False)
    lists = K.make_lists(n, nq, "ragged", 10)
    key_of_row = _key_of_row(n, False)
    se = _index(n, nq, 50, False)
    for thr in (-0.75, 0.0, 0.3):
        keys, scores, counts = _search(se, case[1], _p_keys(lists, key_of_row), k, threshold=thr)
        K.check_by_keys(keys, scores, counts, case, lists, k, thr, None, key_of_row)


def test_a_key_listed_three_times_is_scored_three_times():
    n, nq, k = 5000, 130, 10
    case = R.make_case(n, nq, 50, False)
    _, queries, ref, A, m = case
    B = (m + 1) * 2.0 ** -23 * A
    lists = K.make_lists(n, nq, "ragged", k)
    se = _index(n, nq, 50, False)
    p_keys, best_of = [], {}
    for q in range(nq):
        a = lists[q]
        if len(a) >= 10:
            order = a[np.argsort(ref[q, a], kind="stable")]
            b, second = int(order[0]), int(order[1])
            if ref[q, b] + B[q, b] + B[q, second] < ref[q, second]:          # strictly the best row of its list
                best_of[q] = b
                a = np.concatenate([a[:3], [b], a[3:], [b]])                   # twice more (a lists it once already): three in all
        p_keys.append(a.astype(np.uint64))
    assert len(best_of) >= 10
    keys, scores, counts = _search(se, queries, p_keys, k)
    for q in range(nq):
        c = int(counts[q])
        assert c == min(k, len(p_keys[q]))
        assert np.all(scores[q, 1:c] >= scores[q, :max(c - 1, 0)])
        got = keys[q, :c].astype(np.int64)
        assert set(got.tolist()) <= set(lists[q].tolist())
        assert np.all(np.abs(scores[q, :c].astype(np.float64) - ref[q, got]) <= B[q, got])
        if q in best_of:
            b = best_of[q]
            assert got[:3].tolist() == [b, b, b] and int((got == b).sum()) == 3
            assert scores[q, 0].tobytes() == scores[q, 1].tobytes() == scores[q, 2].tobytes()
            rest = got[3:]
        else:
            rest = got
        assert len(set(rest.tolist())) == len(rest)
    # with room for one candidate only, one of the three copies is returned
    keys1, scores1, counts1 = _search(se, queries, p_keys, 1)
    for q, b in best_of.items():
        assert counts1[q] == 1 and int(keys1[q, 0]) == b and scores1[q, 0].tobytes() == scores[q, 0].tobytes()


def _c_search_by_ids(se, queries, ids, offsets, k, threshold=float(np.finfo(np.float32).max), exclude=None):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    nq = len(queries[0])
    keys = np.full((nq, k if k else 1), 0x1234, np.uint64)           # (sentinels: a refused call leaves them)
    scores = np.full((nq, k if k else 1), -77.0, np.float32)
    counts = np.full(nq, 99, np.uint32)
    qc, qi, qv = (np.ascontiguousarray(x) for x in queries)
    ids = np.ascontiguousarray(ids, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    rc = _lib.lib().zvec_hip_sparse_search_by_ids(se._h, None, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), nq, _np_ptr(ids), _np_ptr(offsets), k,
                                                  float(threshold), _np_ptr(exclude), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
    return rc, keys, scores, counts


def test_c_abi_positions_beyond_the_rows_and_refusals():
    n, nq, k = 65, 65, 10
    case = R.make_case(n, nq, 50, False)
    queries = case[1]
    se = _index(n, nq, 50, False)
    rng = np.random.default_rng(8)
    # every list: 20 distinct rows with positions >= n mixed in (n itself, far beyond, the largest value)
    lists, ids, offsets = [], [], [0]
    for q in range(nq):
        a = rng.permutation(n)[:20]
        lists.append(a)
        b = a.astype(np.int64).tolist()
        for bad in (n, n + 1, 1 << 20, 0xffffffff)[:1 + q % 4]:
            b.insert(int(rng.integers(0, len(b) + 1)), bad)
        ids += b
        offsets.append(len(ids))
    rc, keys, scores, counts = _c_search_by_ids(se, queries, ids, offsets, k)
    assert rc == 0 and counts.tolist() == [k] * nq
    K.check_by_keys(keys, scores, counts, case, lists, k, None, None, np.arange(n, dtype=np.uint64))
    # nothing but positions beyond the rows, with k larger than the lists
    rc, keys, scores, counts = _c_search_by_ids(se, queries, [n, n + 5, 0xffffffff] * nq, np.arange(nq + 1) * 3, 200)
    assert rc == 0 and not counts.any()

    # refusals: InvalidArgument, and no output is touched
    def refused(queries=queries, ids=ids, offsets=offsets, k=k):
        rc, keys, scores, counts = _c_search_by_ids(se, queries, ids, offsets, k)
        assert rc == INVALID
        assert np.all(keys == 0x1234) and np.all(scores == -77.0) and np.all(counts == 99)
    down = list(offsets)
    down[5], down[6] = down[6], down[5]
    refused(offsets=down)                                       # offsets that descend
    refused(offsets=[1] + list(offsets[1:]))                    # offsets[0] != 0
    refused(k=0)
    one = (np.array([2], np.uint32), np.array([5, 4], np.uint32), np.ones(2, np.float32))
    rc, keys, scores, counts = _c_search_by_ids(se, one, [0, 1], [0, 2], k)
    assert rc == INVALID and np.all(keys == 0x1234) and np.all(scores == -77.0) and np.all(counts == 99)
    rc, keys, scores, counts = _c_search_by_ids(se, (np.array([2], np.uint32), np.array([4, 5], np.uint32), np.ones(2, np.float32)), [0, 1], [0, 2], k)
    assert rc == 0 and counts[0] == 2
    rc, _, _, _ = _c_search_by_ids(se, queries, ids, offsets, 5119)
    assert rc == UNSUPPORTED
    from zvec_amd import _lib
    assert _lib.lib().zvec_hip_sparse_search_by_ids(se._h, None, None, None, None, 1, None, None, 1, 0.0, None, None, None, None) == INVALID
    assert _lib.lib().zvec_hip_sparse_batch_distance(None, None, 0, None, None, None, 0, None) == INVALID


def test_python_refusals():
    n, nq = 65, 65
    queries = R.make_case(n, nq, 50, False)[1]
    se = _index(n, nq, 50, False)
    p_keys = [np.arange(3, dtype=np.uint64)] * nq
    ctx = se.create_context()
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys, nq, None) == INVALID
    ctx.set_topk(0)
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys, nq, ctx) == INVALID
    ctx.set_topk(5)
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys[:-1], nq, ctx) == INVALID
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys, nq, ctx) == 0
    ctx.set_group_params(2, 2)
    ctx.set_group_by(lambda key: key % 2)
    assert se.search_bf_by_p_keys_impl(queries[0], queries[1], queries[2], p_keys, nq, ctx) == UNSUPPORTED


def _query(case, q):
    qc, qi, qv = case[1]
    off = R.offsets(qc)
    return qi[off[q]:off[q + 1]], qv[off[q]:off[q + 1]]


@pytest.mark.parametrize("n,nq,vocab,long_queries", [(1000, 1, 100000, True), (65, 65, 50, False), (5000, 130, 50, False)])
def test_batch_distance(n, nq, vocab, long_queries):
    case = R.make_case(n, nq, vocab, long_queries)
    se = _index(n, nq, vocab, long_queries)
    rng = np.random.default_rng(9)
    lengths = {int(case[1][0][q]) for q in range(nq)}
    for q in sorted({0, nq // 2, nq - 1} | {int(np.nonzero(case[1][0] == c)[0][0]) for c in lengths}):
        pos = np.concatenate([rng.permutation(n), rng.integers(0, n, 70), [n, n + 1, 0xffffffff], rng.integers(0, n, 5)]).astype(np.uint32)
        if q % 2:
            pos = pos[:101]                     # (a list that ends inside a slice)
        qi, qv = _query(case, q)
        out = se.batch_distance(qi, qv, pos, se.create_context() if q % 2 else None)
        K.check_batch_distance(out, case, q, pos)
        # a repeated position scores the same bits
        first = {}
        for j, p in enumerate(pos.tolist()):
            assert out[first.setdefault(p, j)].tobytes() == out[j].tobytes()
    qi, qv = _query(case, 0)
    out = se.batch_distance(qi, qv, np.zeros(0, np.uint32))
    assert out.dtype == np.float32 and out.size == 0
    from zvec_amd import _lib
    with pytest.raises(_lib.ZvecHipError):
        se.batch_distance(np.array([5, 4], np.uint32), np.ones(2, np.float32), np.zeros(1, np.uint32))


# A work item takes ceil(listed entries of the call / (16 x CUs)) entries of a list, 64 at most, so only a call with more than
# 63 x 16 x CUs entries (258 048 on 256 CUs) runs full 64-entry slices: lanes 16..63 of the classification, entries picked from the
# upper half of the ballot, the exclude test in those lanes and the full-width store.  Every query lists every row here, about
# 650 000 entries, which is past that for any device of up to 640 CUs.
@pytest.mark.parametrize("k", [10, 200])
def test_full_width_slices(k):
    n, nq = 5000, 130
    case = R.make_case(n, nq, 50, False)
    se = _index(n, nq, 50, False)
    rng = np.random.default_rng(11)
    mask = rng.random(n) < 0.3
    mask[rng.permutation(n)[:64]] = True
    lists, ids, offsets = [], [], [0]
    for q in range(nq):
        a = rng.permutation(n)[:n - q % 5]                # (5000 .. 4996 rows: no multiple of 64, the last slice is partial)
        lists.append(a)
        b = a.astype(np.int64)
        at = np.sort(rng.integers(0, len(b) + 1, 3))
        b = np.insert(b, at, [n, n + 64 + q, 0xffffffff])   # positions beyond the rows, anywhere in the list
        ids.append(b)
        offsets.append(offsets[-1] + len(b))
    ids = np.concatenate(ids)
    assert offsets[-1] > 63 * 16 * 640
    for exclude, words in ((None, None), (mask, _words_of(mask))):
        rc, keys, scores, counts = _c_search_by_ids(se, case[1], ids, offsets, k, exclude=words)
        assert rc == 0
        K.check_by_keys(keys, scores, counts, case, lists, k, None, exclude, np.arange(n, dtype=np.uint64))
    # nothing left but every 64th entry of query 0's list (lanes around 17, 40, 63 of its slices; anywhere in the other lists)
    for lane in (17, 40, 63):
        keep = np.zeros(n, bool)
        keep[lists[0][lane::64]] = True
        rc, keys, scores, counts = _c_search_by_ids(se, case[1], ids, offsets, k, exclude=_words_of(~keep))
        assert rc == 0
        K.check_by_keys(keys, scores, counts, case, lists, k, None, ~keep, np.arange(n, dtype=np.uint64))


def test_batch_distance_full_width_slices():
    n, nq = 5000, 130
    case = R.make_case(n, nq, 50, False)
    se = _index(n, nq, 50, False)
    rng = np.random.default_rng(12)
    pos = rng.integers(0, n, 63 * 16 * 640 + 64 * 100 + 37).astype(np.uint32)         # past the width above, ends inside a slice
    pos[rng.integers(0, pos.size, 500)] = rng.choice(np.array([n, n + 1, 1 << 20, 0xffffffff], np.uint32), 500)
    pos[-1] = n
    for q in (0, nq - 1):
        qi, qv = _query(case, q)
        out = se.batch_distance(qi, qv, pos)
        K.check_batch_distance(out, case, q, pos)
        # a repeated position scores the same bits, whichever lane and slice it fell into
        inside = pos < n
        order = np.argsort(pos[inside], kind="stable")
        p_sorted, bits = pos[inside][order], out[inside][order].view(np.uint32)
        same = p_sorted[1:] == p_sorted[:-1]
        assert np.all(bits[1:][same] == bits[:-1][same])


def test_cross_check_with_the_full_scan():
    n, nq, k = 1000, 64, 10
    case = R.make_case(n, nq, 50, False)
    _, queries, ref, A, m = case
    se = _index(n, nq, 50, False)
    key_of_row = _key_of_row(n, False)
    everything = [np.arange(n, dtype=np.uint64)] * nq
    keys, scores, counts = _search(se, queries, everything, k)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), key_of_row)
    ctx = se.create_context()
    ctx.set_topk(k)
    assert se.search_impl(queries[0], queries[1], queries[2], nq, ctx) == 0
    R.check_sparse_lists(ctx.keys, ctx.scores, ctx.counts, ref, A, m, k, None, np.ones(n, bool), key_of_row)


def test_empty_index_and_empty_lists():
    import zvec_amd as zv
    n, nq = 65, 65
    queries = R.make_case(n, nq, 50, False)[1]
    empty = zv.HipFlatSparseStreamer()
    keys, scores, counts = _search(empty, queries, [np.arange(4, dtype=np.uint64)] * nq, 10)
    assert empty.count() == 0 and not counts.any()
    out = empty.batch_distance(np.array([1, 2], np.uint32), np.ones(2, np.float32), np.array([0, 3], np.uint32))
    assert np.all(np.isposinf(out))
    se = _index(n, nq, 50, False)
    for k in (1, 200):
        keys, scores, counts = _search(se, queries, [np.zeros(0, np.uint64)] * nq, k)
        assert not counts.any()
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search_bf_by_p_keys_impl(queries[0][:0], queries[1][:0], queries[2][:0], [], 0, ctx) == 0

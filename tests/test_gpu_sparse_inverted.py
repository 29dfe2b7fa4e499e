"""Sparse rows under InnerProductSparse searched through the term-major twin (zvec_hip_sparse_set_inverted, zvk_sparse_inv.hip.h),
fp32 and fp16 values, against tests/sparse_ref.py: lists are held to the fp64 reference within B = (m + 1) * 2^-23 * A (derived for
any order of summation, so it covers the twin's term-at-a-time order as it covers the row scan's); integer data must come out bit
for bit.  tests/test_sparse_inverted_reference_cpu.py checks the premises on a numpy model of the twin."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -12, -31
DTYPES = ["fp32", "fp16"]


def _np(dtype):
    return np.float16 if dtype == "fp16" else np.float32


def _index(rows, dtype="fp32", keys=None, pieces=None, inverted=True, metric="InnerProductSparse"):
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
    if inverted:
        se.set_inverted(True)
    _append(se, rows, keys, pieces)
    return se


def _append(se, rows, keys=None, pieces=None, first=0):
    counts, idx, val = rows
    off = R.offsets(counts)
    cuts = [first, len(counts)] if pieces is None else pieces
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], None if keys is None else keys[a:b]) == 0


def _search(se, queries, k, threshold=None, exclude=None, ctx=None):
    ctx = ctx or se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _case(n, nq, vocab, long_queries, dtype):
    """make_case in the index's value type: for fp16 the same runs with every value rounded to half and the reference of those"""
    rows, queries, ref, A, m = R.make_case(n, nq, vocab, long_queries)
    if dtype == "fp16":
        rows = (rows[0], rows[1], rows[2].astype(np.float16))
        queries = (queries[0], queries[1], queries[2].astype(np.float16))
        ref, A = R.sparse_reference((rows[0], rows[1], rows[2].astype(np.float32)), (queries[0], queries[1], queries[2].astype(np.float32)))
    return rows, queries, ref, A, m


def _ints(rng, lengths, vocab, dtype):
    """runs of small non-zero integers, |v| <= 8: products and sums of up to 50 of them are exact in fp32 (and every value in fp16)"""
    counts = np.asarray(lengths, np.uint32)
    idx = [np.sort(rng.choice(vocab, int(c), replace=False)).astype(np.uint32) for c in counts]
    indices = np.concatenate(idx) if idx else np.zeros(0, np.uint32)
    values = (rng.integers(1, 9, indices.size) * rng.choice([-1, 1], indices.size)).astype(_np(dtype))
    return counts, indices, values


def _as32(b):
    return b[0], b[1], b[2].astype(np.float32)


# ---- 1. the band against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nq,vocab,long_queries", [(1000, 65, 50, False), (5000, 64, 100000, True), (20000, 16, 50, False),
                                                      (20000, 16, 100000, False)])
def test_band_against_fp64(n, nq, vocab, long_queries, dtype):
    rows, queries, ref, A, m = _case(n, nq, vocab, long_queries, dtype)
    se = _index(rows, dtype)
    for k in (1, 10, 200):          # (200 is beyond the row scan's fused lists: the twin's route has no such cap)
        keys, scores, counts = _search(se, queries, k)
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))
    info = se.inverted_info()
    assert info["enabled"] and info["builds"] == 1 and info["terms"] == np.unique(rows[1]).size
    assert info["bytes"] >= rows[1].size * (4 + np.dtype(_np(dtype)).itemsize)


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_tile_edges(which, dtype):
    import zvec_amd as zv
    T = zv.HipFlatSparseStreamer(dtype=dtype).inverted_info()["tile_rows"]
    n = (T - 1, T, T + 1, 2 * T + 1)[which]
    special = sorted({r for r in (T - 1, T, 2 * T - 1, 2 * T, n - 1) if 0 <= r < n})
    # every row holds index 7 (one list through every tile) and index 9 on odd rows; the special rows hold the unique best values
    val7 = np.ones(n, np.float32)
    for j, r in enumerate(special):
        val7[r] = 100 + j
    counts = np.where(np.arange(n) % 2 == 1, 2, 1).astype(np.uint32)
    off = R.offsets(counts)
    idx = np.full(off[-1], 7, np.uint32)
    val = np.zeros(off[-1], np.float32)
    val[off[:-1]] = val7
    odd = np.nonzero(counts == 2)[0]
    idx[off[odd] + 1] = 9
    val[off[odd] + 1] = 0.5
    rows = (counts, idx, val.astype(_np(dtype)))
    queries = (np.array([2, 1], np.uint32), np.array([7, 11, 7], np.uint32), np.array([1, 3, 2], _np(dtype)))
    se = _index(rows, dtype)
    k = len(special)
    keys, scores, counts_out = _search(se, queries, k)
    best = sorted(special, key=lambda r: -val7[r])
    assert counts_out.tolist() == [k, k]
    assert keys[0].tolist() == best and keys[1].tolist() == best
    assert scores[0].tolist() == [-float(val7[r]) for r in best] and scores[1].tolist() == [-2 * float(val7[r]) for r in best]
    # one more than the special rows: the next score is the ordinary rows' -1
    keys, scores, counts_out = _search(se, queries, k + 1)
    assert counts_out[0] == min(k + 1, n) and (n == k or scores[0, k] == -1.0)


# ---- 3. integer data, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_data_bit_for_bit(dtype):
    import zvec_amd as zv
    T = zv.HipFlatSparseStreamer().inverted_info()["tile_rows"]
    n, nq, vocab = T + 500, 65, 50
    rng = np.random.default_rng(11)
    rows = _ints(rng, rng.choice([0, 1, 20, 50], n), vocab, dtype)
    queries = _ints(rng, rng.choice([0, 1, 40], nq), vocab, dtype)
    key_of_row = np.arange(n, dtype=np.uint64) * np.uint64(5) + np.uint64(1 << 33)
    exact, _ = R.sparse_reference(_as32(rows), _as32(queries))          # (integers: the fp64 sums are exact)
    exact32 = exact.astype(np.float32)
    assert np.array_equal(exact32.astype(np.float64), exact)
    on = _index(rows, dtype, keys=key_of_row)
    off = _index(rows, dtype, keys=key_of_row, inverted=False)
    row_of_key = {int(key): r for r, key in enumerate(key_of_row)}
    for k in (10, 200):
        want = R.lists_from_scores(exact32, k, None, np.ones(n, bool), key_of_row)
        got_on, got_off = _search(on, queries, k), _search(off, queries, k)
        for got in (got_on, got_off):
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])      # the exact integers, as fp32
        assert np.array_equal(got_on[1], got_off[1])
        for q in range(nq):
            kth = want[1][q, k - 1]
            for got in (got_on, got_off):
                ks = [int(x) for x in got[0][q]]
                assert len(set(ks)) == k
                assert all(exact32[q, row_of_key[key]] == got[1][q, j] for j, key in enumerate(ks))
                # the same keys up to the tie at the k-th place
                assert {x for x, s in zip(ks, got[1][q]) if s < kth} == {int(x) for x, s in zip(want[0][q], want[1][q]) if s < kth}


# ---- 4. zero scores and empties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_scores_and_empties(dtype):
    n, vocab = 3000, 100
    rng = np.random.default_rng(12)
    lengths = rng.choice([0, 1, 5], n)
    lengths[[0, 1, n - 1]] = 0                                         # empty rows at both ends
    rows = _ints(rng, lengths, vocab, dtype)
    rows[2][rows[1] == 3] = np.abs(rows[2][rows[1] == 3])              # index 3 carries positive values only
    holders = int((rows[1] == 3).sum())
    assert 0 < holders < 200
    # a query with no stored term, an empty query, and one that only the holders of index 3 share
    queries = (np.array([2, 0, 2], np.uint32), np.array([5000, 70000, 3, 123456], np.uint32), np.array([1, 2, 1, 4], _np(dtype)))
    ref, A = R.sparse_reference(_as32(rows), _as32(queries))
    m = R.shared_counts(rows, queries)
    se = _index(rows, dtype)
    k = holders + 50
    keys, scores, counts = _search(se, queries, k)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))
    assert counts.tolist() == [k, k, k]
    assert np.all(scores[:2] == 0.0) and not np.signbit(scores[:2]).any()
    assert np.all(scores[2, :holders] < 0.0) and np.all(scores[2, holders:] == 0.0) and not np.signbit(scores[2, holders:]).any()


# ---- 5. exclude bitset and threshold -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [10, 200])
def test_exclude_bitset_and_threshold(k, dtype):
    import zvec_amd as zv
    T = zv.HipFlatSparseStreamer().inverted_info()["tile_rows"]
    n, nq = 2 * T + 1, 16
    rows, queries, ref, A, m = _case(n, nq, 50, False, dtype)
    se = _index(rows, dtype)
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.5
    for edge in (0, 31, 32, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T):      # runs across word and tile boundaries
        mask[max(0, edge - 2):edge + 3] = True
    mask[T + 62:T + 67] = False
    ids = np.arange(n, dtype=np.uint64)
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(mask))
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, ~mask, ids)
    # a threshold half way between the (k/2)-th and the next best score of the longest query cuts inside that query's list
    qs = int(np.argmax(queries[0]))
    best = np.sort(ref[qs])
    inside = float(np.float32((best[k // 2 - 1] + best[k // 2]) / 2))
    B = (m[qs] + 1) * 2.0 ** -23 * A[qs]
    assert best[k // 2] - best[k // 2 - 1] > 4 * B.max() + 2.0 ** -20    # (the two scores are apart by far more than the band)
    for thr in (inside, -0.75, 0.0, 0.3):
        keys, scores, counts = _search(se, queries, k, threshold=thr)
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, thr, np.ones(n, bool), ids)
        if thr == inside:
            assert counts[qs] == k // 2
        keys, scores, counts = _search(se, queries, k, threshold=thr, exclude=_words_of(mask))
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, thr, ~mask, ids)
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(np.ones(n, bool)))
    assert not counts.any()


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_call_twice_same_bits(dtype):
    n, nq = 5000, 64
    rows, queries, _, _, _ = _case(n, nq, 100000, True, dtype)
    se = _index(rows, dtype)
    for k in (10, 200):
        a = _search(se, queries, k)
        b = _search(se, queries, k)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- 7. search_dev on a caller's stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [10, 200])
def test_search_dev_equals_search(k, dtype):
    import torch
    n, nq = 5000, 64
    rows, queries, ref, A, m = _case(n, nq, 100000, True, dtype)
    se = _index(rows, dtype)
    keys, scores, counts = _search(se, queries, k)
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(queries[1].view(np.int32).copy()).to(dev)
    d_val = torch.from_numpy(queries[2].copy()).to(dev)
    d_keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
    d_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d_counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    ctx = se.create_context()
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(2):            # (twice: the second call meets the first one's plan upload)
        assert se.search_dev(queries[0], d_idx.data_ptr(), d_val.data_ptr(), nq, k, d_keys.data_ptr(), d_scores.data_ptr(),
                             d_counts.data_ptr(), ctx, stream=ts.cuda_stream) == 0
    ts.synchronize()
    got_counts = d_counts.cpu().numpy().view(np.uint32)
    got_scores = d_scores.cpu().numpy()
    got_keys = d_keys.cpu().numpy().view(np.uint64)
    assert got_counts.tobytes() == counts.tobytes()
    for q in range(nq):
        c = int(counts[q])
        assert got_scores[q, :c].tobytes() == scores[q, :c].tobytes() and got_keys[q, :c].tobytes() == keys[q, :c].tobytes()
    assert se.inverted_info()["builds"] == 1


# ---- 8. staleness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_appends_mark_stale_and_one_search_rebuilds_once(dtype):
    n, nq, k, n0 = 5000, 63, 10, 4000
    rows, queries, ref, A, m = _case(n, nq, 50, False, dtype)
    ids = np.arange(n, dtype=np.uint64)
    se = _index(rows, dtype, pieces=[0, n0])
    assert se.inverted_info()["builds"] == 0                           # (nothing is built before a search needs it)
    keys, scores, counts = _search(se, queries, k)
    R.check_sparse_lists(keys, scores, counts, ref[:, :n0], A[:, :n0], m[:, :n0], k, None, np.ones(n0, bool), ids[:n0])
    builds = se.inverted_info()["builds"]
    assert builds == 1
    _append(se, rows, pieces=[n0, n0 + 1, n0 + 701, n])
    assert se.count() == n and se.inverted_info()["builds"] == builds  # (neither an append nor the info call builds)
    keys, scores, counts = _search(se, queries, k)
    info = se.inverted_info()
    assert info["builds"] == builds + 1 and info["enabled"] and info["terms"] == np.unique(rows[1]).size
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), ids)
    assert int(counts.min()) == k and int(keys.max()) >= n0            # the new rows are found
    _search(se, queries, k)
    assert se.inverted_info()["builds"] == builds + 1
    # off again: the row scan's answer, and nothing held
    se.set_inverted(False)
    info = se.inverted_info()
    assert not info["enabled"] and info["bytes"] == 0
    plain = _index(rows, dtype, inverted=False)
    a, b = _search(se, queries, k), _search(plain, queries, k)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    R.check_sparse_lists(a[0], a[1], a[2], ref, A, m, k, None, np.ones(n, bool), ids)
    assert se.inverted_info()["builds"] == builds + 1


# ---- 9. the routes that keep reading the rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_listed_and_grouped_routes_are_untouched(dtype):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    L = _lib.lib()
    n, nq, vocab, k = 2000, 5, 50, 10
    rng = np.random.default_rng(13)
    rows = _ints(rng, rng.choice([0, 1, 20], n), vocab, dtype)
    queries = _ints(rng, rng.choice([1, 40], nq), vocab, dtype)
    qc, qi, qv = queries
    lists = [rng.choice(n, 300, replace=False).astype(np.uint32) for _ in range(nq)]
    ids = np.concatenate(lists)
    offs = (np.arange(nq + 1) * 300).astype(np.uint32)
    group_of = rng.integers(0, 20, n).astype(np.uint32)
    fmax = float(np.finfo(np.float32).max)
    answers = []
    for inverted in (True, False):
        se = _index(rows, dtype, inverted=inverted)
        _search(se, queries, k)
        assert se.inverted_info()["builds"] == (1 if inverted else 0)
        ctx = se.create_context()
        by_ids = (np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32))
        assert L.zvec_hip_sparse_search_by_ids(se._h, ctx._h, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), nq, _np_ptr(ids), _np_ptr(offs), k, fmax,
                                               None, *[_np_ptr(a) for a in by_ids]) == 0
        dist = se.batch_distance(qi[:qc[0]], qv[:qc[0]], lists[0], ctx)
        grouped = (np.zeros((nq, 4), np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, 4, 3), np.uint64), np.zeros((nq, 4, 3), np.float32),
                   np.zeros((nq, 4), np.uint32))
        assert L.zvec_hip_sparse_search_grouped(se._h, ctx._h, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), nq, _np_ptr(group_of), 20, 4, 3, fmax,
                                                None, *[_np_ptr(a) for a in grouped]) == 0
        gi, gv = se.get_vector_by_id(n - 1)
        answers.append([a.tobytes() for a in by_ids + (dist,) + grouped + (gi, gv)])
    assert answers[0] == answers[1]


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    from zvec_amd import _lib
    L = _lib.lib()
    rows, queries, ref, A, m = R.make_case(1000, 65, 50, False)
    # SquaredEuclideanSparse: refused, and the handle answers as before
    l2 = _index(rows, inverted=False, metric="SquaredEuclideanSparse")
    before = _search(l2, queries, 10)
    assert L.zvec_hip_sparse_set_inverted(l2._h, 1) == UNSUPPORTED
    info = l2.inverted_info()
    assert not info["enabled"] and info["bytes"] == 0 and info["builds"] == 0
    after = _search(l2, queries, 10)
    assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
    # a NULL handle
    assert L.zvec_hip_sparse_set_inverted(None, 1) == INVALID and L.zvec_hip_sparse_set_inverted(None, 0) == INVALID
    assert L.zvec_hip_sparse_inverted_info(None, None, None, None, None, None) == INVALID
    # topk beyond the merge cap, with the twin on
    se = _index(rows)
    ctx = se.create_context()
    ctx.set_topk(5119)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == UNSUPPORTED
    ctx.set_topk(5118)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
    assert ctx.counts.tolist() == [1000] * 65
    # every output of the info call is optional
    assert L.zvec_hip_sparse_inverted_info(se._h, None, None, None, None, None) == 0
    tile = C.c_uint32(0)
    assert L.zvec_hip_sparse_inverted_info(se._h, None, None, None, C.byref(tile), None) == 0 and tile.value > 0

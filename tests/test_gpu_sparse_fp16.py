"""Sparse fp16 rows under InnerProductSparse on the GPU (zvec_hip_sparse_create_typed(ZVEC_HIP_DT_FP16, ...)), against the fp64
reference of tests/sparse_ref.py on the cases of tests/sparse_fp16_ref.py: values rounded to half, the reference recomputed on the
rounded values, the band B = (m + 1) * 2^-23 * A unchanged (a product of two halves is exact in fp32).  Integer data and single
products are compared bit for bit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_fp16_ref as H  # noqa: E402
import sparse_keys_ref as K  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID, NO_EXIST = -12, -31, -22
FMAX = float(np.finfo(np.float32).max)


def _index(rows, keys=None, pieces=None, dtype="fp16"):
    """an index of `rows`; an fp16 one is handed float16 arrays"""
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer(dtype=dtype)
    counts, idx, val = H.halves(rows) if dtype == "fp16" else rows
    off = R.offsets(counts)
    cuts = [0, len(counts)] if pieces is None else pieces
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], None if keys is None else keys[a:b]) == 0
    assert se.count() == len(counts) and se.element_count() == int(off[-1])
    return se


@functools.lru_cache(maxsize=None)
def _shared_index(kind, *args):
    """one index per case for the tests that do not change it"""
    return _index((H.make_integer_case if kind == "int" else H.make_case)(*args)[0])


def _search(se, queries, k, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    qc, qi, qv = H.halves(queries)
    assert se.search_impl(qc, qi, qv, len(qc), ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _assert_same_answer(a, b, k):
    """two searches of the same index gave the same answer: counts, score bits, and the keys wherever the interface fixes them.
    Which of several rows with EQUAL scores are returned at the k-th place, and the order of equal scores, is unspecified
    (include/zvec_hip.h, Ties) and on the fused route depends on which chunk publishes its bound first, so of a full list only the
    entries strictly better than its last score are compared, as (score, key) pairs in any order; a list shorter than k holds every
    candidate, so all of it is."""
    (ka, sa, ca), (kb, sb, cb) = a, b
    assert np.asarray(ca).tolist() == np.asarray(cb).tolist()
    for q in range(len(ca)):
        c = int(ca[q])
        assert sa[q, :c].tobytes() == sb[q, :c].tobytes()
        fixed = c if c < k else int(np.count_nonzero(sa[q, :c] < sa[q, c - 1]))
        pairs = [sorted(zip(s[q, :fixed].view(np.uint32).tolist(), kk[q, :fixed].tolist())) for kk, s in ((ka, sa), (kb, sb))]
        assert pairs[0] == pairs[1], q


def _dtype_of_handle(se):
    from zvec_amd import _lib
    d = C.c_int(-1)
    assert _lib.lib().zvec_hip_sparse_dtype(se._h, C.byref(d)) == 0
    return d.value


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,vocab,k,long_queries", R.CASES)
def test_against_the_reference(n, nq, vocab, k, long_queries):
    rows, queries, ref, A, m = H.make_case(n, nq, vocab, long_queries)
    k = n + 5 if k == "n+5" else k
    se = _index(rows)
    assert _dtype_of_handle(se) == 1
    keys, scores, counts = _search(se, queries, k)
    assert scores.dtype == np.float32
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


# ---- 2. exact sums far beyond half range -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 200])
@pytest.mark.parametrize("nq", [1, 64, 65])
def test_integer_sums_beyond_half_range_are_exact(nq, k):
    rows, queries, ref, A, m = H.make_integer_case(nq)
    n = H.INT_N
    key_of_row = np.arange(n, dtype=np.uint64)
    keys, scores, counts = _search(_shared_index("int", nq), queries, k)
    assert counts.tolist() == [min(k, n)] * nq
    H.assert_exact(keys, scores, counts, ref, key_of_row)
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, np.ones(n, bool), key_of_row)
    # exact arithmetic leaves nothing free but the order of equal scores: the list is the k smallest reference scores
    want = np.sort(ref, axis=1)[:, :min(k, n)].astype(np.float32)
    assert scores[:, :min(k, n)].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert scores[0, 0] == -262144.0


# ---- 3. edge values, one product per pair ------------------------------------------------------------------------------------------
EDGE = np.array([2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, -0.0, 1.0], np.float16)


def _edge_batches():
    """row r / query q: (index 5, EDGE[r]) and one index nobody else has; then a row sharing nothing and an empty row"""
    e = len(EDGE)
    rows = (np.array([2] * e + [1, 0], np.uint32),
            np.concatenate([np.array([[5, 100 + r] for r in range(e)], np.uint32).reshape(-1), [300]]).astype(np.uint32),
            np.concatenate([np.stack([EDGE, np.ones(e, np.float16)], 1).reshape(-1), np.array([3.0], np.float16)]))
    queries = (np.array([2] * e, np.uint32), np.array([[5, 200 + q] for q in range(e)], np.uint32).reshape(-1),
               np.stack([EDGE, np.full(e, 2.0, np.float16)], 1).reshape(-1))
    return rows, queries


def _edge_expected():
    e = len(EDGE)
    v = EDGE.astype(np.float32)
    want = np.zeros((e, e + 2), np.float32)                      # (no shared index: +0.0)
    with np.errstate(over="raise", under="raise"):
        for q in range(e):
            for r in range(e):
                p = np.float32(v[q] * v[r])                      # exact: 11 x 11 significant bits, |p| in [2^-48, 2^32) or 0
                assert float(p) == float(v[q]) * float(v[r])
                want[q, r] = np.float32(0) - (np.float32(0) + p)     # the sum starts at +0, so a -0 product leaves +0
    return want


def test_edge_values_one_product_per_pair():
    import zvec_amd as zv
    rows, queries = _edge_batches()
    want = _edge_expected()
    assert want[0, 0] == np.float32(-(2.0 ** -48)) and want[2, 2] == np.float32(-(65504.0 ** 2)) and want[2, 3] == np.float32(65504.0 ** 2)
    assert want[4, 5].tobytes() == np.float32(0.0).tobytes() and want[0, 1] == np.float32(-(2.0 ** -38))
    se = zv.HipFlatSparseStreamer(dtype="fp16")
    assert se.add_batch(*rows) == 0
    n = len(rows[0])
    ctx = se.create_context()
    for k in (n, 200):                                           # the fused lists and the dense-score route
        ctx.set_topk(k)
        assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
        assert ctx.counts.tolist() == [n] * len(EDGE)
        for q in range(len(EDGE)):
            got = ctx.scores[q, :n]
            pos = ctx.keys[q, :n].astype(np.int64)
            assert sorted(pos.tolist()) == list(range(n))
            assert got.view(np.uint32).tolist() == want[q, pos].view(np.uint32).tolist(), (q, got, want[q, pos])
            assert np.all(got[1:] >= got[:-1])
    # listed rows: the same bits, in the listed order
    for q in range(len(EDGE)):
        out = se.batch_distance(queries[1][2 * q:2 * q + 2], queries[2][2 * q:2 * q + 2], np.arange(n, dtype=np.uint32))
        assert out.view(np.uint32).tolist() == want[q].view(np.uint32).tolist(), (q, out, want[q])


# ---- 4. listed rows ----------------------------------------------------------------------------------------------------------------
LIST_LENGTHS = (0, 1, 63, 64, 65, 200)


def _lists(n, nq, seed):
    rng = np.random.default_rng([seed, n, nq])
    return [rng.permutation(n)[:LIST_LENGTHS[q % 6]].astype(np.int64) for q in range(nq)]


def _c_search_by_ids(se, queries, ids, offsets, k, exclude=None):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    qc, qi, qv = (np.ascontiguousarray(x) for x in H.halves(queries))
    nq = len(qc)
    keys = np.zeros((nq, k), np.uint64)
    scores = np.zeros((nq, k), np.float32)
    counts = np.zeros(nq, np.uint32)
    ids = np.ascontiguousarray(ids, np.uint32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    rc = _lib.lib().zvec_hip_sparse_search_by_ids(se._h, None, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), nq, _np_ptr(ids), _np_ptr(offsets), k,
                                                  FMAX, _np_ptr(exclude), _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
    assert rc == 0
    return keys, scores, counts


@pytest.mark.parametrize("k", [10, 500])
@pytest.mark.parametrize("n,nq,vocab,long_queries", [(1000, 64, 50, False), (1000, 65, 100000, True)])
def test_search_by_ids_against_the_reference(n, nq, vocab, long_queries, k):
    case = H.make_case(n, nq, vocab, long_queries)
    se = _shared_index("case", n, nq, vocab, long_queries)
    lists = _lists(n, nq, 1)
    key_of_row = np.arange(n, dtype=np.uint64)
    qc, qi, qv = H.halves(case[1])
    mask = np.random.default_rng(2).random(n) < 0.4
    for excluded in (None, mask):
        ctx = se.create_context()
        ctx.set_topk(k)
        if excluded is not None:
            ctx.set_exclude_bitset(_words_of(excluded))
        assert se.search_bf_by_p_keys_impl(qc, qi, qv, [key_of_row[a] for a in lists], nq, ctx) == 0
        alive = [a if excluded is None else a[~excluded[a]] for a in lists]
        assert ctx.counts.tolist() == [min(k, len(a)) for a in alive]
        K.check_by_keys(ctx.keys, ctx.scores, ctx.counts, case, lists, k, None, excluded, key_of_row)
        # positions beyond the rows anywhere in the list, and every entry listed twice: the beyond ones are never returned, a row
        # listed twice is scored twice with the same bits, and the first copies are an answer to the plain lists
        rng = np.random.default_rng(3)
        ids, offsets = [], [0]
        for a in lists:
            b = np.concatenate([a, a])
            b = np.insert(b, np.sort(rng.integers(0, len(b) + 1, 3)), [n, n + 64, 0xffffffff])
            ids.append(b)
            offsets.append(offsets[-1] + len(b))
        keys, scores, counts = _c_search_by_ids(se, case[1], np.concatenate(ids), offsets, k,
                                                None if excluded is None else _words_of(excluded))
        assert counts.tolist() == [min(k, 2 * len(a)) for a in alive]
        # The first copies: a full list of k entries holds both copies of every row strictly better than its last entry, so its
        # first k // 2 distinct keys are a top-(k // 2) answer to the plain lists; a shorter list holds every live row twice.
        kk = k // 2
        dk = np.full((nq, kk), 0xffffffffffffffff, np.uint64)
        ds = np.zeros((nq, kk), np.float32)
        dc = np.zeros(nq, np.uint32)
        for q in range(nq):
            c = int(counts[q])
            assert np.all(scores[q, 1:c] >= scores[q, :max(c - 1, 0)])
            seen = {}
            for j, key in enumerate(keys[q, :c].tolist()):
                seen.setdefault(key, []).append(j)
            for js in seen.values():
                assert len(js) <= 2 and scores[q, js[0]].tobytes() == scores[q, js[-1]].tobytes()
                assert len(js) == 2 or c == k
            first = [js[0] for js in seen.values()][:kk]
            dc[q] = len(first)
            dk[q, :len(first)] = keys[q, first]
            ds[q, :len(first)] = scores[q, first]
        K.check_by_keys(dk, ds, dc, case, lists, kk, None, excluded, key_of_row)


@pytest.mark.parametrize("n,nq,vocab,long_queries", [(1000, 64, 50, False), (1000, 65, 100000, True)])
def test_batch_distance_against_the_reference(n, nq, vocab, long_queries):
    case = H.make_case(n, nq, vocab, long_queries)
    se = _shared_index("case", n, nq, vocab, long_queries)
    rng = np.random.default_rng(9)
    qc, qi, qv = H.halves(case[1])
    qo = R.offsets(qc)
    picked = sorted({0, nq - 1} | {int(np.nonzero(qc == c)[0][0]) for c in set(qc.tolist())})
    for j, q in enumerate(picked):
        length = LIST_LENGTHS[j % 6]
        pos = np.concatenate([rng.integers(0, n, length), rng.integers(0, n, length // 2), [n, 0xffffffff][:min(length, 2)]]).astype(np.uint32)
        out = se.batch_distance(qi[qo[q]:qo[q + 1]], qv[qo[q]:qo[q + 1]], pos, se.create_context() if q % 2 else None)
        K.check_batch_distance(out, case, q, pos)
    pos = np.concatenate([rng.permutation(n)[:200], [n + 1], rng.integers(0, n, 60)]).astype(np.uint32)     # duplicates, 261 entries
    for q in picked[:3]:
        out = se.batch_distance(qi[qo[q]:qo[q + 1]], qv[qo[q]:qo[q + 1]], pos)
        K.check_batch_distance(out, case, q, pos)
        first = {}
        for j, p in enumerate(pos.tolist()):
            assert out[first.setdefault(p, j)].tobytes() == out[j].tobytes()


@pytest.mark.parametrize("k", [10, 500])
def test_listed_rows_of_the_integer_data_are_exact(k):
    nq, n = 65, H.INT_N
    case = H.make_integer_case(nq)
    ref = case[2]
    se = _shared_index("int", nq)
    rng = np.random.default_rng(4)
    ids, offsets = [], [0]
    for q in range(nq):
        ids.append(rng.integers(0, n + 10, LIST_LENGTHS[q % 6]))         # duplicates and positions beyond the rows
        offsets.append(offsets[-1] + len(ids[-1]))
    mask = rng.random(n) < 0.3
    for excluded in (None, mask):
        keys, scores, counts = _c_search_by_ids(se, case[1], np.concatenate(ids), offsets, k,
                                                None if excluded is None else _words_of(excluded))
        H.assert_exact(keys, scores, counts, ref, np.arange(n, dtype=np.uint64))
        for q in range(nq):
            a = ids[q][ids[q] < n]
            if excluded is not None:
                a = a[~excluded[a]]
            want = np.sort(ref[q, a])[:k].astype(np.float32)           # exact arithmetic: the k smallest, duplicates counted
            assert counts[q] == want.size
            assert scores[q, :want.size].view(np.uint32).tolist() == want.view(np.uint32).tolist()
            assert set(keys[q, :want.size].tolist()) <= set(a.tolist())
    qc, qi, qv = H.halves(case[1])
    qo = R.offsets(qc)
    pos = np.concatenate([rng.integers(0, n + 10, 200), np.arange(n)]).astype(np.uint32)
    for q in (0, 1, 2, 63, 64):
        out = se.batch_distance(qi[qo[q]:qo[q + 1]], qv[qo[q]:qo[q + 1]], pos)
        want = np.where(pos < n, ref[q, np.minimum(pos, n - 1)], np.inf).astype(np.float32)
        assert out.view(np.uint32).tolist() == want.view(np.uint32).tolist()
        K.check_batch_distance(out, case, q, pos)


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------------
def test_get_vector_round_trip_of_arbitrary_finite_halves():
    import zvec_amd as zv
    rng = np.random.default_rng(6)
    counts = np.array([0, 1, 65, 4096, 1, 0, 65, 4096, 3], np.uint32)
    idx = np.concatenate([np.sort(rng.choice(1 << 20, int(c), replace=False)) for c in counts]).astype(np.uint32)
    bits = rng.integers(0, 1 << 16, idx.size).astype(np.uint16)
    bits[(bits & 0x7c00) == 0x7c00] &= np.uint16(0xbfff)         # (no inf, no NaN: clear one exponent bit)
    bits[:8] = [0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff, 0xfbff, 0x8000, 0x0000][:8]     # subnormals, the largest, both zeros
    val = bits.view(np.float16)
    assert np.isfinite(val).all()
    off = R.offsets(counts)
    se = zv.HipFlatSparseStreamer(dtype="fp16")
    for a, b in zip([0, 1, 4, 6], [1, 4, 6, 9]):                 # pieces of unequal size; the store grows in between
        assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]]) == 0
    assert se.count() == counts.size and se.element_count() == idx.size
    for pos in range(counts.size):
        gi, gv = se.get_vector_by_id(pos)
        assert gi.dtype == np.uint32 and gv.dtype == np.float16 and gi.size == gv.size == counts[pos]
        assert gi.tolist() == idx[off[pos]:off[pos + 1]].tolist()
        assert gv.view(np.uint16).tolist() == bits[off[pos]:off[pos + 1]].tolist()
    assert se.get_vector_by_id(counts.size) is None
    from zvec_amd import _lib
    c = C.c_uint32(77)
    assert _lib.lib().zvec_hip_sparse_get_vector(se._h, 3, C.byref(c), None, None) == 0 and c.value == 4096
    assert _lib.lib().zvec_hip_sparse_get_vector(se._h, counts.size, C.byref(c), None, None) == NO_EXIST


# ---- 6. threshold and exclude bitset -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 200])
def test_threshold(k):
    n, nq = 1000, 64
    rows, queries, ref, A, m = H.make_case(n, nq, 50, False)
    se = _shared_index("case", n, nq, 50, False)
    for thr in (-0.75, 0.0, 0.3):
        keys, scores, counts = _search(se, queries, k, threshold=thr)
        R.check_sparse_lists(keys, scores, counts, ref, A, m, k, thr, np.ones(n, bool), np.arange(n, dtype=np.uint64))
    assert int(counts.max()) == k


@pytest.mark.parametrize("k", [10, 200])
def test_exclude_bitset_across_chunk_boundaries(k):
    n, nq = 5000, 65
    rows, queries, ref, A, m = H.make_case(n, nq, 50, False)
    se = _shared_index("case", n, nq, 50, False)
    rng = np.random.default_rng(5)
    mask = rng.random(n) < 0.5
    mask[0:130] = True            # whole chunks of rows, and runs that straddle every chunk boundary near them
    mask[2499:2503] = True
    mask[-1] = True
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(mask))
    R.check_sparse_lists(keys, scores, counts, ref, A, m, k, None, ~mask, np.arange(n, dtype=np.uint64))
    keys, scores, counts = _search(se, queries, k, exclude=_words_of(np.ones(n, bool)))
    assert not counts.any()


# ---- 7. search_dev equals search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 200])
def test_search_dev_equals_search(k):
    import torch
    n, nq = 1000, 130
    rows, queries, ref, A, m = H.make_case(n, nq, 100000, True)
    se = _shared_index("case", n, nq, 100000, True)
    keys, scores, counts = _search(se, queries, k)
    qc, qi, qv = H.halves(queries)
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(qi.view(np.int32).copy()).to(dev)
    d_val = torch.from_numpy(qv.copy()).to(dev)
    assert d_val.dtype == torch.float16 and d_val.element_size() == 2
    d_keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
    d_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d_counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    ctx = se.create_context()
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(2):            # (twice: the second call meets the first one's plan upload)
        assert se.search_dev(qc, d_idx.data_ptr(), d_val.data_ptr(), nq, k, d_keys.data_ptr(), d_scores.data_ptr(),
                             d_counts.data_ptr(), ctx, stream=ts.cuda_stream) == 0
    ts.synchronize()
    got_counts = d_counts.cpu().numpy().view(np.uint32)
    got_scores = d_scores.cpu().numpy()
    got_keys = d_keys.cpu().numpy().view(np.uint64)
    _assert_same_answer((got_keys, got_scores, got_counts), (keys, scores, counts), k)
    R.check_sparse_lists(got_keys, got_scores, got_counts, ref, A, m, k, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))


# ---- 8. fp32 through the new door --------------------------------------------------------------------------------------------------
def test_fp32_through_create_typed_equals_create():
    import zvec_amd as zv
    from zvec_amd import _lib
    n, nq, k = 1000, 65, 10
    rows, queries, ref, A, m = R.make_case(n, nq, 100000, True)
    typed = _index(rows, dtype="fp32")                         # zvec_hip_sparse_create_typed(ZVEC_HIP_DT_FP32, ...)
    plain = zv.HipFlatSparseStreamer.__new__(zv.HipFlatSparseStreamer)      # ... and one from zvec_hip_sparse_create
    plain.device, plain.dtype, plain.np_dtype, plain._keys_host, plain._h = 0, _lib.DT_FP32, np.float32, [], C.c_void_p()
    assert _lib.lib().zvec_hip_sparse_create(0, C.byref(plain._h)) == 0
    assert plain.add_batch(*rows) == 0
    assert _dtype_of_handle(typed) == _lib.DT_FP32 and _dtype_of_handle(plain) == _lib.DT_FP32
    assert _dtype_of_handle(_shared_index("int", 1)) == _lib.DT_FP16
    for kk in (k, 200):
        out = []
        for se in (typed, plain):
            ctx = se.create_context()
            ctx.set_topk(kk)
            assert se.search_impl(queries[0], queries[1], queries[2], nq, ctx) == 0
            out.append((ctx.keys.copy(), ctx.scores.copy(), ctx.counts.copy()))
        _assert_same_answer(out[0], out[1], kk)
        for o in out:
            R.check_sparse_lists(*o, ref, A, m, kk, None, np.ones(n, bool), np.arange(n, dtype=np.uint64))
    gi, gv = typed.get_vector_by_id(0)
    assert gv.dtype == np.float32 and gv.tobytes() == rows[2][:rows[0][0]].tobytes()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    L = _lib.lib()
    out = C.c_void_p(0x55)
    for bad in (_lib.DT_BINARY32, _lib.DT_BINARY64, 4, -1):
        assert L.zvec_hip_sparse_create_typed(bad, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    assert L.zvec_hip_sparse_create_typed(_lib.DT_FP16, 0, None) == INVALID
    with pytest.raises(_lib.ZvecHipError):
        zv.HipFlatSparseStreamer(dtype="binary32")
    se = zv.HipFlatSparseStreamer(dtype="fp16")
    d = C.c_int(-1)
    assert L.zvec_hip_sparse_dtype(se._h, None) == INVALID and L.zvec_hip_sparse_dtype(None, C.byref(d)) == INVALID
    ok = (np.array([2, 0, 1], np.uint32), np.array([3, 9, 4], np.uint32), np.ones(3, np.float16))
    assert se.add_batch(*ok) == 0 and se.count() == 3
    # NULL values with elements to read
    c1, i1 = np.array([1], np.uint32), np.array([9], np.uint32)
    assert L.zvec_hip_sparse_append(se._h, _np_ptr(c1), _np_ptr(i1), None, 1, None) == INVALID
    keys, scores, counts = np.zeros((1, 2), np.uint64), np.zeros((1, 2), np.float32), np.zeros(1, np.uint32)
    assert L.zvec_hip_sparse_search(se._h, None, _np_ptr(c1), _np_ptr(i1), None, 1, 2, FMAX, None, _np_ptr(keys), _np_ptr(scores),
                                    _np_ptr(counts)) == INVALID
    assert L.zvec_hip_sparse_batch_distance(se._h, None, 1, _np_ptr(i1), None, _np_ptr(np.zeros(1, np.uint32)), 1, _np_ptr(scores)) == INVALID
    # a run of 4097 elements, an unsorted run, a repeated index: InvalidArgument, and nothing of the call is stored
    long_idx = np.arange(4097, dtype=np.uint32)
    assert se.add_batch(np.array([1, 4097], np.uint32), np.concatenate([[5], long_idx]).astype(np.uint32), np.ones(4098, np.float16)) == INVALID
    assert se.add_batch(np.array([1, 2], np.uint32), np.array([7, 9, 8], np.uint32), np.ones(3, np.float16)) == INVALID
    assert se.add_batch(np.array([2], np.uint32), np.array([8, 8], np.uint32), np.ones(2, np.float16)) == INVALID
    assert se.count() == 3 and se.element_count() == 3
    ctx = se.create_context()
    ctx.set_topk(2)
    assert se.search_impl(np.array([4097], np.uint32), long_idx, np.ones(4097, np.float16), 1, ctx) == INVALID
    assert se.search_impl(np.array([2], np.uint32), np.array([5, 4], np.uint32), np.ones(2, np.float16), 1, ctx) == INVALID
    # other float inputs are cast to half
    assert se.search_impl(c1, i1, np.ones(1, np.float64), 1, ctx) == 0
    assert ctx.counts[0] == 2 and int(ctx.keys[0, 0]) == 0 and ctx.scores[0].tolist() == [-1.0, 0.0]
    assert se.search_impl(c1, np.array([3], np.uint32), np.full(1, 0.5, np.float32), 1, ctx) == 0
    assert ctx.counts[0] == 2 and int(ctx.keys[0, 0]) == 0 and ctx.scores[0].tolist() == [-0.5, 0.0]
    ctx.set_topk(5119)
    assert se.search_impl(c1, i1, np.ones(1, np.float16), 1, ctx) == UNSUPPORTED

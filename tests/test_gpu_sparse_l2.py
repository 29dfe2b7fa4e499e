"""Sparse rows under SquaredEuclideanSparse on the GPU (zvec_hip_sparse_create_metric(.., ZVEC_HIP_METRIC_L2, ..)), through the C ABI
and HipFlatSparseStreamer, for fp32 and fp16 values, against the fp64 reference and the band of tests/sparse_l2_ref.py.  For fp16 the
inputs are rounded to halves first, so the reference sees what is stored.  Integer data is held bit for bit on every route; a row
searched with itself scores exactly +0.0 on every route."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_group_ref as G  # noqa: E402
import sparse_l2_ref as L  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -12, -31
FMAX = float(np.finfo(np.float32).max)
DTYPES = ["fp32", "fp16"]
NP = {"fp32": np.float32, "fp16": np.float16}
L2, IP = "SquaredEuclideanSparse", "InnerProductSparse"
PLUS_ZERO = np.float32(0.0).tobytes()


def _lib():
    from zvec_amd import _lib as M
    return M.lib()


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _cast(batch, dtype):
    c, i, v = batch
    return np.ascontiguousarray(c, np.uint32), np.ascontiguousarray(i, np.uint32), np.ascontiguousarray(v).astype(NP[dtype])


def _key_of(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)


def _index(rows, dtype, metric=L2):
    """an index of `rows` (already of the value type), keys = position * 3 + 7, appended in two pieces"""
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
    assert se.metric == metric
    counts, idx, val = _cast(rows, dtype)
    assert np.array_equal(val.astype(np.float64), np.asarray(rows[2]).astype(np.float64)), "the case's values are not of the index's type"
    n = len(counts)
    off = R.offsets(counts)
    keys = _key_of(n)
    for a, b in ((0, n // 2), (n // 2, n)):
        if b > a:
            assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], keys[a:b]) == 0
    assert se.count() == n and se.element_count() == int(off[-1])
    return se


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _outs(nq, k):
    return np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)


def _search(se, dtype, queries, k, threshold=None, exclude=None):
    """zvec_hip_sparse_search"""
    qc, qi, qv = _cast(queries, dtype)
    keys, scores, counts = _outs(len(qc), k)
    ex = None if exclude is None else _words_of(exclude)
    rc = _lib().zvec_hip_sparse_search(se._h, None, _ptr(qc), _ptr(qi), _ptr(qv), len(qc), k, FMAX if threshold is None else threshold,
                                       _ptr(ex), _ptr(keys), _ptr(scores), _ptr(counts))
    assert rc == 0
    return keys, scores, counts


def _search_dev(se, dtype, queries, k, exclude=None):
    """zvec_hip_sparse_search_dev on a stream of its own"""
    import torch
    qc, qi, qv = _cast(queries, dtype)
    nq = len(qc)
    dev = torch.device("cuda:0")
    d_idx = torch.from_numpy(np.concatenate([qi, np.zeros(1, np.uint32)]).view(np.int32).copy()).to(dev)
    d_val = torch.from_numpy(np.concatenate([qv, np.zeros(1, qv.dtype)])).to(dev)
    d_ex = None if exclude is None else torch.from_numpy(_words_of(exclude).view(np.int64).copy()).to(dev)
    d_keys = torch.empty((nq, k), dtype=torch.int64, device=dev)
    d_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    d_counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    ts = torch.cuda.Stream(device=dev)
    ts.wait_stream(torch.cuda.current_stream(dev))
    assert se.search_dev(qc, d_idx.data_ptr(), d_val.data_ptr(), nq, k, d_keys.data_ptr(), d_scores.data_ptr(), d_counts.data_ptr(),
                         se.create_context(), d_exclude=None if d_ex is None else d_ex.data_ptr(), stream=ts.cuda_stream) == 0
    ts.synchronize()
    return d_keys.cpu().numpy().view(np.uint64), d_scores.cpu().numpy(), d_counts.cpu().numpy().view(np.uint32)


def _flat_lists(lists):
    ids = np.concatenate([np.asarray(a, np.uint32) for a in lists] + [np.zeros(1, np.uint32)]).astype(np.uint32)
    offs = np.zeros(len(lists) + 1, np.uint32)
    offs[1:] = np.cumsum([len(a) for a in lists])
    return ids, offs


def _by_ids(se, dtype, queries, lists, k, exclude=None):
    """zvec_hip_sparse_search_by_ids"""
    qc, qi, qv = _cast(queries, dtype)
    keys, scores, counts = _outs(len(qc), k)
    ids, offs = _flat_lists(lists)
    ex = None if exclude is None else _words_of(exclude)
    rc = _lib().zvec_hip_sparse_search_by_ids(se._h, None, _ptr(qc), _ptr(qi), _ptr(qv), len(qc), _ptr(ids), _ptr(offs), k, FMAX, _ptr(ex),
                                              _ptr(keys), _ptr(scores), _ptr(counts))
    assert rc == 0
    return keys, scores, counts


def _batch_distance(se, dtype, queries, q, positions):
    qc, qi, qv = _cast(queries, dtype)
    o = R.offsets(qc)
    return se.batch_distance(qi[o[q]:o[q + 1]], qv[o[q]:o[q + 1]], np.asarray(positions, np.uint32))


@contextlib.contextmanager
def _group_rows(value):
    """"sparse_group_rows" set to `value`, the previous value restored afterwards"""
    lib = _lib()
    before = C.c_int(-1)
    assert lib.zvec_hip_get_option(b"sparse_group_rows", C.byref(before)) == 0
    assert lib.zvec_hip_set_option(b"sparse_group_rows", value) == 0
    try:
        yield
    finally:
        assert lib.zvec_hip_set_option(b"sparse_group_rows", before.value) == 0


def _grouped(se, dtype, queries, gof, ng, gnum, gk, exclude=None, lists=None):
    """zvec_hip_sparse_search_grouped / _grouped_by_ids: (groups, ngroups, keys, scores, counts)"""
    qc, qi, qv = _cast(queries, dtype)
    nq = len(qc)
    out = (np.zeros((nq, gnum), np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, gnum, gk), np.uint64),
           np.zeros((nq, gnum, gk), np.float32), np.zeros((nq, gnum), np.uint32))
    gof = np.ascontiguousarray(gof, np.uint32)
    ex = None if exclude is None else _words_of(exclude)
    if lists is None:
        rc = _lib().zvec_hip_sparse_search_grouped(se._h, None, _ptr(qc), _ptr(qi), _ptr(qv), nq, _ptr(gof), ng, gnum, gk, FMAX, _ptr(ex),
                                                   *[_ptr(a) for a in out])
    else:
        ids, offs = _flat_lists(lists)
        rc = _lib().zvec_hip_sparse_search_grouped_by_ids(se._h, None, _ptr(qc), _ptr(qi), _ptr(qv), nq, _ptr(ids), _ptr(offs), _ptr(gof),
                                                          ng, gnum, gk, FMAX, _ptr(ex), *[_ptr(a) for a in out])
    assert rc == 0
    return out


def _assert_bits(keys, scores, counts, want32, n):
    """every returned score is, bit for bit, the wanted fp32 score of the row its key names"""
    row_of_key = {int(k): r for r, k in enumerate(_key_of(n))}
    for q in range(len(counts)):
        c = int(counts[q])
        rows = [row_of_key[int(x)] for x in keys[q, :c]]
        assert scores[q, :c].view(np.uint32).tolist() == want32[q, rows].view(np.uint32).tolist(), q


# ---- 1. band cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,vocab,k,long_queries", R.CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_band_cases(dtype, n, nq, vocab, k, long_queries):
    rows, queries, ref = L.make_l2_case(n, nq, vocab, long_queries, dtype == "fp16")
    k = n + 5 if k == "n+5" else k
    se = _index(rows, dtype)
    key_of_row = _key_of(n)
    keys, scores, counts = _search(se, dtype, queries, k)
    L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, np.ones(n, bool), key_of_row)
    mask = np.zeros(n, bool)
    mask[::3] = True
    thr = float(np.float32(np.median(ref["score"])))
    keys, scores, counts = _search(se, dtype, queries, k, threshold=thr, exclude=mask)
    L.check_sparse_l2_lists(keys, scores, counts, ref, k, thr, ~mask, key_of_row)


# ---- 2. exact integer cases ----------------------------------------------------------------------------------------------------------
_INT = {}


def _integer_case(which):
    """(rows, queries, ref, want32): non-zero integers in [-3, 3], so every sum is exact in fp32 (at most 8192 terms of at most 36
    is below 2^24).  "short": n = 130, nq = 66, vocabulary 50, runs of 0 / 1 / 20 / 50; "long": n = 70, nq = 5, vocabulary 5000,
    runs of 64 / 65 / 4096 with several rows and two queries of 4096 (pairs share thousands of indices)"""
    if which not in _INT:
        rng = np.random.default_rng([31, len(which)])
        if which == "short":
            n, nq, vocab = 130, 66, 50
            rl, ql = rng.choice([0, 1, 20, 50], n), rng.choice([0, 1, 20, 50], nq)
            rl[:4], ql[:4] = [0, 1, 20, 50], [50, 0, 1, 20]
        else:
            n, nq, vocab = 70, 5, 5000
            rl = rng.choice([64, 65], n)
            rl[[0, 37, 69]] = 4096
            ql = np.array([4096, 64, 4096, 65, 64])

        def runs(lengths):
            c, i, _ = R.random_runs(rng, lengths, vocab)
            return c, i, rng.choice([-3, -2, -1, 1, 2, 3], i.size).astype(np.float32)

        rows, queries = runs(rl), runs(ql)
        ref = L.sparse_l2_reference(rows, queries)
        want32 = ref["score"].astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), ref["score"]) and ref["score"].max() < 2 ** 24
        _INT[which] = (rows, queries, ref, want32)
    return _INT[which]


def _exact_lists(rng, n, nq, mask):
    """per query a list with a position >= n, a position listed twice and an excluded position; one list is empty"""
    lists = []
    for q in range(nq):
        a = rng.integers(0, n, (0, 5, 40, 64, 65, 150)[(q + 2) % 6])
        if a.size:
            a = np.concatenate([a, [n + q, a[0], np.nonzero(mask)[0][q % 7], 0xffffffff]])
        lists.append(rng.permutation(a).astype(np.uint32))
    assert any(a.size == 0 for a in lists)
    return lists


@pytest.mark.parametrize("which", ["short", "long"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_integer_cases(dtype, which):
    rows, queries, ref, want32 = _integer_case(which)
    n, nq = len(rows[0]), len(queries[0])
    se = _index(rows, dtype)
    key_of_row = _key_of(n)
    rng = np.random.default_rng(32)
    mask = rng.random(n) < 0.3
    lists = _exact_lists(rng, n, nq, mask)
    for k in (1, 10, n + 5):
        # search and search_dev
        for excluded in (None, mask):
            for route in (_search, _search_dev):
                keys, scores, counts = route(se, dtype, queries, k, exclude=excluded)
                alive = np.ones(n, bool) if excluded is None else ~excluded
                assert counts.tolist() == [min(k, int(alive.sum()))] * nq
                L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, alive, key_of_row, exact=True)
                _assert_bits(keys, scores, counts, want32, n)
        # search_by_ids: the k smallest of the live entries, a position listed twice counted twice
        for excluded in (None, mask):
            keys, scores, counts = _by_ids(se, dtype, queries, lists, k, excluded)
            _assert_bits(keys, scores, counts, want32, n)
            for q in range(nq):
                a = lists[q][lists[q] < n].astype(np.int64)
                if excluded is not None:
                    a = a[~excluded[a]]
                want = np.sort(want32[q, a])[:k]
                assert counts[q] == want.size
                assert scores[q, :want.size].view(np.uint32).tolist() == want.view(np.uint32).tolist()
                assert set(keys[q, :want.size].tolist()) <= set(key_of_row[a].tolist())
    # batch_distance: the listed order, +inf for a position beyond the rows
    pos = np.concatenate([rng.integers(0, n, 90), [n, 0xffffffff], np.arange(n)]).astype(np.uint32)
    for q in range(min(nq, 6)):
        out = _batch_distance(se, dtype, queries, q, pos)
        want = np.where(pos < n, want32[q, np.minimum(pos, n - 1)], np.float32(np.inf)).astype(np.float32)
        assert out.view(np.uint32).tolist() == want.view(np.uint32).tolist(), q
    # group-by: 7 groups, 3 groups of 2 documents, one position whose group is beyond the groups; the selection logic of
    # tests/sparse_group_ref.py applied to the L2 score matrix
    ng, gnum, gk = 7, 3, 2
    gof = rng.integers(0, ng, n).astype(np.uint32)
    gof[n // 2] = ng
    sub = list(range(min(nq, 64)))                     # (at most 64 queries: "sparse_group_rows" 64 takes them a wave per row)
    qsub = G.take_queries(queries, sub)
    for excluded in (None, mask):
        want = G.render(G.select(want32[sub], gof, ng, gnum, gk, None, excluded), gnum, gk, key_of_row)
        for w in (0, 64):
            with _group_rows(w):
                got = _grouped(se, dtype, qsub, gof, ng, gnum, gk, excluded)
            G.check_exact(want, got, "%s rows=%d" % (which, w))
        want = G.render(G.select(want32, gof, ng, gnum, gk, None, excluded, candidates=lists), gnum, gk, key_of_row)
        G.check_exact(want, _grouped(se, dtype, queries, gof, ng, gnum, gk, excluded, lists=lists), "%s by ids" % which)


# ---- 3. a row searched with itself ---------------------------------------------------------------------------------------------------
SELF_LENGTHS = (1, 20, 64, 65, 300, 4096)


def _self_rows(dtype):
    rng = np.random.default_rng(33)
    c, i, v = R.random_runs(rng, [SELF_LENGTHS[r % 6] for r in range(65)], 6000)
    v = rng.standard_normal(v.size).astype(np.float32) * np.float32(1.7)
    return c, i, v.astype(NP[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_self_query_scores_plus_zero_on_every_route(dtype):
    rows = _self_rows(dtype)
    n = 65
    ro = R.offsets(rows[0])
    assert len({(rows[1][ro[r]:ro[r + 1]].tobytes(), rows[2][ro[r]:ro[r + 1]].tobytes()) for r in range(n)}) == n, "rows not distinct"
    ref = L.sparse_l2_reference(rows, rows)
    assert not np.diag(ref["score"]).any() and np.count_nonzero(ref["score"] == 0) == n
    se = _index(rows, dtype)
    key_of_row = _key_of(n)

    def first_is_self(keys, scores, counts):
        for q in range(n):
            assert counts[q] >= 1 and int(keys[q, 0]) == int(key_of_row[q]), q
            assert scores[q, 0].tobytes() == PLUS_ZERO, (q, scores[q, 0])

    rng = np.random.default_rng(34)
    lists = [rng.permutation(np.concatenate([rng.integers(0, n, 30), [q, n + 3]])).astype(np.uint32) for q in range(n)]
    for k in (1, 10, n + 5):
        for route in (_search, _search_dev):
            keys, scores, counts = route(se, dtype, rows, k)
            first_is_self(keys, scores, counts)
            L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, np.ones(n, bool), key_of_row)
        first_is_self(*_by_ids(se, dtype, rows, lists, k))
    for q in range(n):
        out = _batch_distance(se, dtype, rows, q, [q])
        assert out.tobytes() == PLUS_ZERO, (q, out)
    ng, gnum, gk = 7, 3, 2
    gof = rng.integers(0, ng, n).astype(np.uint32)
    first64 = G.take_queries((rows[0], rows[1], rows[2].astype(np.float32)), range(64))
    answers = []
    for w in (0, 64):
        with _group_rows(w):
            answers.append((64, _grouped(se, dtype, first64, gof, ng, gnum, gk)))
    answers.append((n, _grouped(se, dtype, rows, gof, ng, gnum, gk, lists=lists)))
    for count, (groups, ngroups, keys, scores, counts) in answers:
        for q in range(count):
            assert ngroups[q] >= 1 and groups[q, 0] == gof[q] and counts[q, 0] >= 1, q
            assert int(keys[q, 0, 0]) == int(key_of_row[q]) and scores[q, 0, 0].tobytes() == PLUS_ZERO, (q, scores[q, 0, 0])


# ---- 4. covered queries: every query element meets one of the row ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_covered_queries_are_held_to_the_row_side_band_alone(dtype):
    rng = np.random.default_rng(35)
    n = 36
    c, i, v = R.random_runs(rng, [SELF_LENGTHS[r % 6] for r in range(n)], 6000)
    rows = (c, i, v.astype(NP[dtype]))
    ro = R.offsets(c)
    qidx = []
    for r in range(n):                                 # a subset of row r's indices (all of them for every 4th row), fresh values
        own = i[ro[r]:ro[r + 1]]
        take = own.size if r % 4 == 0 else max(1, own.size // 2)
        qidx.append(np.sort(rng.choice(own, take, replace=False)).astype(np.uint32))
    qi = np.concatenate(qidx)
    queries = (np.array([a.size for a in qidx], np.uint32), qi, rng.uniform(-1.0, 1.0, qi.size).astype(np.float32).astype(NP[dtype]))
    ref = L.sparse_l2_reference(rows, queries)
    d = np.arange(n)
    assert np.array_equal(ref["hits"][d, d], ref["qlen"][d, d])
    row_side = (ref["rlen"] + 4) * 2.0 ** -23 * ref["A64"]
    assert np.array_equal(L.band(ref)[d, d], row_side[d, d]) and np.all(row_side[d, d] > 0)
    assert np.any(L.band(ref) > row_side)              # (the other pairs do carry the query-side term)
    se = _index(rows, dtype)
    key_of_row = _key_of(n)
    for k in (n, n + 100):                             # the fused lists and the dense-score route
        keys, scores, counts = _search(se, dtype, queries, k)
        assert counts.tolist() == [n] * n
        L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, np.ones(n, bool), key_of_row)
        for q in range(n):
            j = keys[q, :n].tolist().index(int(key_of_row[q]))
            assert abs(float(scores[q, j]) - ref["score"][q, q]) <= row_side[q, q], (q, scores[q, j], ref["score"][q, q], row_side[q, q])
    for q in range(n):
        out = _batch_distance(se, dtype, queries, q, [q])
        assert abs(float(out[0]) - ref["score"][q, q]) <= row_side[q, q], (q, out[0], ref["score"][q, q], row_side[q, q])


# ---- 5. no overlap, empties, threshold -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_overlap_empties_and_threshold(dtype):
    rng = np.random.default_rng(36)
    n, nq = 40, 6
    # (one empty row: every empty row scores the same Qn, and the threshold part below wants distinct scores at the first ranks)
    c, i, v = R.random_runs(rng, [0] + [(1, 20, 64, 65, 300)[r % 5] for r in range(n - 1)], 1000)
    rows = (c, i, v.astype(NP[dtype]))
    qc, qi, qv = R.random_runs(rng, [40, 0, 1, 65, 300, 7], 1000)
    queries = (qc, qi + np.uint32(2000), qv.astype(NP[dtype]))
    ref = L.sparse_l2_reference(rows, queries)
    assert not ref["hits"].any()
    # an empty row scores Qn, an empty query the row's A, both empty exactly 0; nothing else is 0
    assert np.array_equal(ref["score"][:, 0], ref["Q64"][:, 0]) and np.array_equal(ref["score"][1], ref["A64"][1])
    both = (ref["rlen"] == 0) & (ref["qlen"] == 0)
    assert both.sum() == 1 and np.array_equal(ref["score"] == 0, both)
    se = _index(rows, dtype)
    key_of_row = _key_of(n)
    for k in (n, n + 100):                             # the fused lists and the dense-score route
        keys, scores, counts = _search(se, dtype, queries, k)
        assert counts.tolist() == [n] * nq
        L.check_sparse_l2_lists(keys, scores, counts, ref, k, None, np.ones(n, bool), key_of_row)
        row_of_key = {int(x): r for r, x in enumerate(key_of_row)}
        for q in range(nq):
            for j in range(n):
                r = row_of_key[int(keys[q, j])]
                assert (scores[q, j].tobytes() == PLUS_ZERO) == bool(both[q, r]), (q, r, scores[q, j])
                assert both[q, r] or scores[q, j] > 0
    out = _batch_distance(se, dtype, queries, 1, np.arange(n))        # the empty query: every row's own squares
    assert np.all(np.abs(out.astype(np.float64) - ref["A64"][1]) <= L.band(ref)[1]) and out[0].tobytes() == PLUS_ZERO
    # threshold: non-strict at the fp32 score of rank 3
    k = 10
    keys, scores, counts = _search(se, dtype, queries, k)
    for q in (0, 3):
        s3, key3 = scores[q, 2], int(keys[q, 2])
        assert scores[q, 1] < s3 < scores[q, 3]
        kk, ss, cc = _search(se, dtype, queries, k, threshold=float(s3))
        assert cc[q] == 3 and int(kk[q, 2]) == key3 and ss[q, 2].tobytes() == s3.tobytes()
        kk, ss, cc = _search(se, dtype, queries, k, threshold=float(np.nextafter(s3, np.float32(-np.inf))))
        assert cc[q] == 2 and key3 not in kk[q, :2].tolist()


# ---- 6. surface --------------------------------------------------------------------------------------------------------------------------
def _metric_of(h):
    m = C.c_int(-1)
    assert _lib().zvec_hip_sparse_metric(h, C.byref(m)) == 0
    return m.value


@pytest.mark.parametrize("dtype", DTYPES)
def test_surface(dtype):
    import zvec_amd as zv
    from zvec_amd import _lib as M
    lib = M.lib()
    dt = M.DT_FP16 if dtype == "fp16" else M.DT_FP32
    made = []
    h = C.c_void_p()
    assert lib.zvec_hip_sparse_create(0, C.byref(h)) == 0
    made.append(h)
    assert _metric_of(h) == M.METRIC_IP
    h = C.c_void_p()
    assert lib.zvec_hip_sparse_create_typed(dt, 0, C.byref(h)) == 0
    made.append(h)
    assert _metric_of(h) == M.METRIC_IP
    for metric in (M.METRIC_L2, M.METRIC_IP):
        h = C.c_void_p()
        assert lib.zvec_hip_sparse_create_metric(dt, metric, 0, C.byref(h)) == 0
        made.append(h)
        assert _metric_of(h) == metric
        d = C.c_int(-1)
        assert lib.zvec_hip_sparse_dtype(h, C.byref(d)) == 0 and d.value == dt
    m = C.c_int(-1)
    assert lib.zvec_hip_sparse_metric(made[0], None) == INVALID and lib.zvec_hip_sparse_metric(None, C.byref(m)) == INVALID
    out = C.c_void_p(0x55)
    for bad in (M.METRIC_COSINE, M.METRIC_HAMMING, 7):
        assert lib.zvec_hip_sparse_create_metric(dt, bad, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    for bad in (M.DT_BINARY32, M.DT_BINARY64):
        for metric in (M.METRIC_L2, M.METRIC_IP, M.METRIC_HAMMING):
            assert lib.zvec_hip_sparse_create_metric(bad, metric, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    assert lib.zvec_hip_sparse_create_metric(dt, M.METRIC_L2, 0, None) == INVALID
    for h in made:
        assert lib.zvec_hip_sparse_destroy(h) == 0
    with pytest.raises(ValueError):
        zv.HipFlatSparseStreamer(dtype=dtype, metric="MipsSquaredEuclideanSparse")
    assert zv.HipFlatSparseStreamer(dtype=dtype).metric == IP
    # create_metric(.., METRIC_IP, ..) and create_typed are the same kernels: one vocabulary-50 case, identical key and score bits
    n, nq, k = 1000, 64, 10
    rows, queries = R.make_case(n, nq, 50, False)[:2]
    rows, queries = [(c, i, v.astype(NP[dtype])) for c, i, v in (rows, queries)]
    by_metric = _index(rows, dtype, IP)
    assert _metric_of(by_metric._h) == M.METRIC_IP
    typed = zv.HipFlatSparseStreamer.__new__(zv.HipFlatSparseStreamer)
    typed.device, typed.dtype, typed.np_dtype, typed._keys_host, typed._h = 0, dt, NP[dtype], [], C.c_void_p()
    assert lib.zvec_hip_sparse_create_typed(dt, 0, C.byref(typed._h)) == 0
    c, i, v = _cast(rows, dtype)
    assert typed.add_batch(c, i, v, _key_of(n)) == 0
    for kk in (k, 200):                                # the fused lists and the dense-score route
        a, b = _search(by_metric, dtype, queries, kk), _search(typed, dtype, queries, kk)
        assert a[2].tolist() == b[2].tolist()
        for q in range(nq):
            cq = int(a[2][q])
            assert a[1][q, :cq].tobytes() == b[1][q, :cq].tobytes(), q
            fixed = cq if cq < kk else int(np.count_nonzero(a[1][q, :cq] < a[1][q, cq - 1]))      # (ties at the k-th place are free)
            assert sorted(zip(a[1][q, :fixed].view(np.uint32).tolist(), a[0][q, :fixed].tolist())) == sorted(
                zip(b[1][q, :fixed].view(np.uint32).tolist(), b[0][q, :fixed].tolist())), q
    # get_vector on an L2 handle: rows bit for bit
    se = _index(rows, dtype)
    ro = R.offsets(c)
    for pos in (0, 1, 2, 3, n - 1):
        gi, gv = se.get_vector_by_id(pos)
        assert gi.tolist() == i[ro[pos]:ro[pos + 1]].tolist() and gv.dtype == NP[dtype]
        assert gv.tobytes() == v[ro[pos]:ro[pos + 1]].tobytes()
    assert se.get_vector_by_id(n) is None

"""The sparse index fed from device memory (zvec_hip_sparse_append_dev, _append_dense_dev, _from_dense_dev, _search_dense_dev,
_ingest_info) against the numpy reference of tests/sparse_ingest_ref.py and against the host entries.  Everything is bit for bit:
the converter is exact and ordered, and two handles that hold the same store run the same kernels on it.  Both value types; both
metrics wherever a search is involved."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ingest_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_OF_RANGE, INVALID, UNSUPPORTED = -17, -31, -12
FLT_MAX = G.FLT_MAX
DTYPES = ["fp32", "fp16"]
METRICS = ["InnerProductSparse", "SquaredEuclideanSparse"]
NP = {"fp32": np.float32, "fp16": np.float16}
DT = {"fp32": 0, "fp16": 1}
VOCAB = 30522
INVALID_KEY = np.uint64(0xffffffffffffffff)


def _lib():
    from zvec_amd import _lib as L
    return L.lib()


def _new(dtype, metric="InnerProductSparse"):
    import zvec_amd as zv
    return zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)


def _dev(a):
    """a numpy array as a torch tensor on the GPU holding the same bits (unsigned words as signed ones)"""
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    t = torch.from_numpy((a.view(signed) if signed else a).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def _matrix(rng, n, dim, dt, density):
    """random rows with the edges in them: an all-zero row, non-zeros only in the first / only in the last column, -0.0 and
    subnormal entries"""
    m = np.where(rng.random((n, dim)) < density, rng.uniform(-1.0, 1.0, (n, dim)), 0.0).astype(dt)
    sub = np.array([1, 3], np.uint16 if dt is np.float16 else np.uint32).view(dt)
    for r in range(n):
        kind = r % 7
        if kind == 1:
            m[r] = 0.0
        elif kind == 2:
            m[r] = 0.0
            m[r, 0] = 0.5
        elif kind == 3:
            m[r] = 0.0
            m[r, dim - 1] = -0.25
        elif kind == 4:
            m[r, rng.integers(0, dim)] = -0.0
            m[r, rng.integers(0, dim)] = sub[0]
            m[r, dim - 1] = -sub[1]
    return m


def _padded(m, ld, off):
    """the matrix inside a buffer whose rows are ld elements apart and start `off` elements in; everything around the rows is 7.0,
    which would be kept if it were read"""
    n, dim = m.shape
    buf = np.full(off + max(n * ld, 1), 7.0, m.dtype)
    buf[off:off + n * ld].reshape(n, ld)[:, :dim] = m
    return buf


def _append_dense(se, m, ld=None, off=0, keys=None):
    n, dim = m.shape
    ld = dim if ld is None else ld
    d = _dev(_padded(m, ld, off))
    k = None if keys is None else _dev(np.asarray(keys, np.uint64))
    return _lib().zvec_hip_sparse_append_dense_dev(se._h, _p(d, off), n, dim, ld, _p(k), None)


def _append_csr(se, csr, keys=None, elements=None):
    c, i, v = csr
    dc, di, dv = _dev(np.asarray(c, np.uint32)), _dev(np.asarray(i, np.uint32)), _dev(v)
    k = None if keys is None else _dev(np.asarray(keys, np.uint64))
    return _lib().zvec_hip_sparse_append_dev(se._h, _p(dc), _p(di), _p(dv), len(c), len(i) if elements is None else elements, _p(k), None)


def _search(se, csr, k):
    ctx = se.create_context()
    ctx.set_topk(k)
    c, i, v = csr
    assert se.search_impl(c, i, v, len(c), ctx) == 0
    return ctx.keys.tobytes(), ctx.scores.tobytes(), ctx.counts.tobytes()


def _info(se):
    return se.ingest_info()


# ---- 1. a dense append equals the host append of the reference's CSR ----------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_append_equals_host_append(dtype, dim):
    dt = NP[dtype]
    rng = np.random.default_rng([1, dim, DT[dtype]])
    density = 0.5 if dim == 1 else min(0.3, 40.0 / dim + 0.05)
    queries = G.dense_to_csr(_matrix(rng, 5, dim, dt, density))
    # (rows, extra elements between rows, elements in front): every row distance and the shifted base at 65 rows, the other row
    # counts with one distance each
    cases = [(65, pad, off) for pad in (0, 1, 3) for off in (0, 1)] + [(1, 1, 1), (2, 3, 0), (300, 1, 1)]
    for j, (n, pad, off) in enumerate(cases):
        metric = METRICS[j % 2]
        m = _matrix(rng, n, dim, dt, density)
        csr = G.dense_to_csr(m)
        keys = None if j % 3 else np.arange(n, dtype=np.uint64) * 3 + 11
        a, b = _new(dtype, metric), _new(dtype, metric)
        assert _append_dense(a, m, dim + pad, off, keys) == 0, (n, pad, off)
        assert b.add_batch(*csr, keys=keys) == 0
        G.assert_same_store(G.read_store(a), G.read_store(b))
        assert _search(a, queries, 10) == _search(b, queries, 10), (n, pad, off, metric)
        assert _info(a)["route"] == 1 and _info(a)["elements"] == csr[1].size


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_at_the_cap_and_a_narrow_wide_call(dtype):
    dt = NP[dtype]
    rng = np.random.default_rng([2, DT[dtype]])
    full = rng.uniform(0.5, 1.0, (2, 4096)).astype(dt)         # every column non-zero: exactly the cap
    full[1, 5:] = 0.0
    a, b = _new(dtype), _new(dtype)
    assert _append_dense(a, full) == 0 and b.add_batch(*G.dense_to_csr(full)) == 0
    G.assert_same_store(G.read_store(a), G.read_store(b))
    assert a.get_vector_by_id(0)[0].size == 4096
    # three rows over the whole vocabulary, about 100 non-zeros each: rows cut into column slices
    assert 0 < _info(a)["slice_cols"] < VOCAB
    wide = np.zeros((3, VOCAB), dt)
    for r in range(3):
        cols = rng.choice(VOCAB, 100, replace=False)
        wide[r, cols] = rng.uniform(0.1, 1.0, 100).astype(dt)
    wide[2, VOCAB - 1] = 1.0
    wide[1, 0] = -1.0
    for metric in METRICS:
        a, b = _new(dtype, metric), _new(dtype, metric)
        assert _append_dense(a, wide, VOCAB + 1, 1) == 0 and b.add_batch(*G.dense_to_csr(wide)) == 0
        G.assert_same_store(G.read_store(a), G.read_store(b))
        q = G.dense_to_csr(wide[:2])
        assert _search(a, q, 3) == _search(b, q, 3)
    # no column at all: empty rows
    a = _new(dtype)
    assert _append_dense(a, np.zeros((4, 0), dt)) == 0 and a.count() == 4 and a.element_count() == 0


# ---- 2. a CSR append on the device equals the host append -------------------------------------------------------------------------
def _csr_batch(rng, n, dim, dt):
    return G.dense_to_csr(_matrix(rng, n, dim, dt, 0.1))


@pytest.mark.parametrize("with_keys", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_append_on_the_device_equals_host_append(dtype, with_keys):
    dt = NP[dtype]
    rng = np.random.default_rng([3, DT[dtype], int(with_keys)])
    for metric in METRICS:
        a, b = _new(dtype, metric), _new(dtype, metric)
        assert a.reserve(4, 16) == 0 and b.reserve(4, 16) == 0          # (the second batch grows the store)
        base = 0
        for n in (3, 70, 1):                                             # onto an empty handle, then onto one with rows
            csr = _csr_batch(rng, n, 500, dt)
            keys = (np.arange(n, dtype=np.uint64) + base) * 5 + 2 if with_keys else None
            assert _append_csr(a, csr, keys) == 0
            assert b.add_batch(*csr, keys=keys) == 0
            base += n
            G.assert_same_store(G.read_store(a), G.read_store(b))
            assert _info(a)["route"] == 0 and _info(a)["elements"] == csr[1].size
        assert _lib().zvec_hip_sparse_append_dev(a._h, None, None, None, 0, 0, None, None) == 0 and a.count() == base      # n == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_append_onto_a_handle_with_holes(dtype):
    dt = NP[dtype]
    rng = np.random.default_rng([4, DT[dtype]])
    first = _csr_batch(rng, 2, 500, dt)
    a, b = _new(dtype), _new(dtype)
    for se in (a, b):
        assert se.add_with_id_batch([3, 7], *first) == 0                 # holes at 0, 1, 2 and 4, 5, 6
    assert a.holes() == 6
    csr = _csr_batch(rng, 130, 500, dt)
    dense = _matrix(rng, 9, 500, dt, 0.1)
    assert _append_csr(a, csr) == 0 and b.add_batch(*csr) == 0
    assert _append_dense(a, dense, 503, 1) == 0 and b.add_batch(*G.dense_to_csr(dense)) == 0
    assert a.holes() == 6 and a.count() == 8 + 130 + 9
    G.assert_same_store(G.read_store(a), G.read_store(b))
    keys, _, counts = G.search_all(a)                                    # every row ties at 0: a hole would be admitted if it were scored
    assert int(counts[0]) == a.count() - 6 and not (keys[0, :int(counts[0])] == INVALID_KEY).any()


# ---- 3. refusals leave the store untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_calls_change_nothing(dtype):
    dt = NP[dtype]
    rng = np.random.default_rng([5, DT[dtype]])
    se = _new(dtype)
    se.set_inverted(True)
    assert se.add_with_id_batch([2], *_csr_batch(rng, 1, 300, dt)) == 0  # (two holes)
    assert _append_csr(se, _csr_batch(rng, 20, 300, dt)) == 0
    query = _csr_batch(rng, 2, 300, dt)
    before_search = _search(se, query, 5)
    before = G.read_store(se)
    builds = se.inverted_info()["builds"]
    info = _info(se)
    L = _lib()
    one = np.ones(1, dt)

    def val(n):
        return np.ones(n, dt)

    bad = [
        ([3, 2], [1, 4, 4, 0, 9], None),                                 # a run with an equal neighbour
        ([3, 2], [1, 4, 9, 5, 2], None),                                 # a descending pair at a run's last element
        ([2, 4097], np.concatenate([[0, 1], np.arange(4097)]), None),    # a count of 4097
        ([2, 3], [1, 4, 0, 2, 9], 6),                                    # counts summing to elements - 1
        ([2, 3], [1, 4, 0, 2, 9, 11], 4),                                # ... and to elements + 1
    ]
    for counts, idx, elements in bad:
        idx = np.asarray(idx, np.uint32)
        assert G.check_csr(counts, idx, elements) == INVALID
        pairs = max(idx.size, elements or 0)
        idx = np.concatenate([idx, np.arange(idx.size, pairs, dtype=np.uint32) + 100000])
        assert _append_csr(se, (counts, idx, val(pairs)), elements=elements) == INVALID, (counts, elements)
    m = _matrix(rng, 6, 4200, dt, 0.02)
    m[4, :4097] = 1.0                                                    # 4097 non-zeros among good rows
    assert _append_dense(se, m) == INVALID
    good = _dev(_matrix(rng, 3, 40, dt, 0.3))
    cnt = _dev(np.array([1], np.uint32))
    assert L.zvec_hip_sparse_append_dense_dev(se._h, _p(good), 3, 40, 39, None, None) == INVALID       # ld < dim
    assert L.zvec_hip_sparse_append_dense_dev(se._h, None, 3, 40, 40, None, None) == INVALID
    assert L.zvec_hip_sparse_append_dense_dev(None, _p(good), 3, 40, 40, None, None) == INVALID
    assert L.zvec_hip_sparse_append_dev(se._h, None, _p(cnt), _p(_dev(one)), 1, 1, None, None) == INVALID
    assert L.zvec_hip_sparse_append_dev(se._h, _p(cnt), None, _p(_dev(one)), 1, 1, None, None) == INVALID
    assert L.zvec_hip_sparse_append_dev(se._h, _p(cnt), _p(cnt), None, 1, 1, None, None) == INVALID
    assert L.zvec_hip_sparse_append_dev(None, _p(cnt), _p(cnt), _p(_dev(one)), 1, 1, None, None) == INVALID
    assert _info(se) == info                                             # the last SUCCESSFUL call
    assert _search(se, query, 5) == before_search
    assert se.inverted_info()["builds"] == builds                        # nothing went out of date
    G.assert_same_store(before, G.read_store(se))


# ---- 4. the converter alone -----------------------------------------------------------------------------------------------------------
def _from_dense(ctx, dtype, d, off, n, dim, ld, d_counts, d_idx, d_val, cap):
    total = C.c_uint64(12345)
    rc = _lib().zvec_hip_sparse_from_dense_dev(ctx._h, DT[dtype], _p(d, off), n, dim, ld, _p(d_counts), _p(d_idx), _p(d_val), cap,
                                               C.byref(total), None)
    ctx.synchronize()
    return rc, int(total.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_from_dense_size_query_fill_and_capacity(dtype):
    import zvec_amd as zv
    dt = NP[dtype]
    rng = np.random.default_rng([6, DT[dtype]])
    n, dim, ld, off = 37, 5003, 5006, 1
    m = _matrix(rng, n, dim, dt, 0.03)
    m[6] = rng.uniform(0.5, 1.0, dim).astype(dt)                         # 5000 non-zeros: converted, not refused
    m[6, [3, 1003, 2003]] = 0.0
    counts, idx, val = G.dense_to_csr(m)
    assert counts[6] == 5000
    ctx = zv.IndexContext(0)
    d = _dev(_padded(m, ld, off))
    d_counts = _dev(np.full(n, 0xdeadbeef, np.uint32))
    rc, total = _from_dense(ctx, dtype, d, off, n, dim, ld, d_counts, None, None, 0)
    assert rc == 0 and total == idx.size and np.array_equal(_host(d_counts), counts)
    pat_i, pat_v = np.full(idx.size + 8, 0xabababab, np.uint32), np.full(idx.size + 8, 3.0, dt)
    d_idx, d_val = _dev(pat_i), _dev(pat_v)
    rc, total = _from_dense(ctx, dtype, d, off, n, dim, ld, d_counts, d_idx, d_val, idx.size - 1)
    assert rc == OUT_OF_RANGE and total == idx.size
    assert np.array_equal(_host(d_idx), pat_i) and G.raw(_host(d_val)).tobytes() == G.raw(pat_v).tobytes()
    rc, total = _from_dense(ctx, dtype, d, off, n, dim, ld, d_counts, d_idx, d_val, idx.size)
    assert rc == 0 and total == idx.size and np.array_equal(_host(d_counts), counts)
    got_i, got_v = _host(d_idx), _host(d_val)
    assert np.array_equal(got_i[:idx.size], idx) and G.raw(got_v[:idx.size]).tobytes() == G.raw(val).tobytes()
    assert np.array_equal(got_i[idx.size:], pat_i[idx.size:])            # nothing behind the pairs
    # the same bits on every call
    d_idx2, d_val2 = _dev(pat_i), _dev(pat_v)
    assert _from_dense(ctx, dtype, d, off, n, dim, ld, d_counts, d_idx2, d_val2, idx.size + 8)[0] == 0
    assert np.array_equal(_host(d_idx2), got_i) and G.raw(_host(d_val2)).tobytes() == G.raw(got_v).tobytes()
    # refusals
    total = C.c_uint64(7)
    L = _lib()
    assert L.zvec_hip_sparse_from_dense_dev(ctx._h, 2, _p(d), n, dim, ld, _p(d_counts), None, None, 0, C.byref(total), None) == UNSUPPORTED
    assert L.zvec_hip_sparse_from_dense_dev(ctx._h, DT[dtype], _p(d), n, dim, dim - 1, _p(d_counts), None, None, 0, C.byref(total),
                                            None) == INVALID
    assert L.zvec_hip_sparse_from_dense_dev(ctx._h, DT[dtype], None, n, dim, ld, _p(d_counts), None, None, 0, C.byref(total), None) == INVALID
    assert L.zvec_hip_sparse_from_dense_dev(ctx._h, DT[dtype], _p(d), n, dim, ld, None, None, None, 0, C.byref(total), None) == INVALID
    assert L.zvec_hip_sparse_from_dense_dev(None, DT[dtype], _p(d), n, dim, ld, _p(d_counts), None, None, 0, C.byref(total), None) == INVALID
    assert total.value == 0


# ---- 5. dense queries equal the CSR search of the reference's CSR -------------------------------------------------------------------
def _search_dev_pair(se, qm, ld, off, k, threshold, exclude):
    """(dense-query search, CSR search of the same queries): keys, scores, counts of each, as bytes"""
    count, dim = qm.shape
    ctx = se.create_context()
    d = _dev(_padded(qm, ld, off))
    c, i, v = G.dense_to_csr(qm)
    di, dv = _dev(i), _dev(v)
    ex = None if exclude is None else _dev(exclude)
    outs = []
    for dense in (True, False):
        keys, scores, cnts = _dev(np.full((count, k), 99, np.uint64)), _dev(np.full((count, k), 9.0, np.float32)), _dev(np.full(count, 77, np.uint32))
        if dense:
            rc = _lib().zvec_hip_sparse_search_dense_dev(se._h, ctx._h, _p(d, off), count, dim, ld, k, threshold, _p(ex), _p(keys),
                                                         _p(scores), _p(cnts), None)
        else:
            rc = se.search_dev(c, di.data_ptr(), dv.data_ptr(), count, k, keys.data_ptr(), scores.data_ptr(), cnts.data_ptr(), ctx,
                               threshold=threshold, d_exclude=ex.data_ptr() if ex is not None else None)
        assert rc == 0
        ctx.synchronize()
        outs.append((_host(keys).tobytes(), _host(scores).tobytes(), _host(cnts).tobytes()))
    return outs


# (the inverted lists serve the inner product only)
@pytest.mark.parametrize("metric,inverted", [(METRICS[0], False), (METRICS[0], True), (METRICS[1], False)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_queries_equal_the_csr_search(dtype, metric, inverted):
    dt = NP[dtype]
    rng = np.random.default_rng([7, DT[dtype], METRICS.index(metric)])
    n, dim = 700, 1500
    se = _new(dtype, metric)
    rows = _matrix(rng, n, dim, dt, 0.02)
    assert _append_dense(se, rows) == 0
    if inverted:
        se.set_inverted(True)
    exclude = rng.integers(0, 2 ** 63, (n + 63) // 64, dtype=np.uint64)
    finite = -0.05 if metric == "InnerProductSparse" else 12.0
    for count in (1, 33):
        qm = _matrix(rng, count, dim, dt, 0.03)
        qm[count // 2] = 0.0                                             # a query that is all zeros
        for k, threshold, ex in ((10, FLT_MAX, None), (7, finite, exclude), (200, FLT_MAX, exclude)):
            dense, csr = _search_dev_pair(se, qm, dim + 3, 1, k, threshold, ex)
            assert dense == csr, (count, k, threshold)
    # a query with 4097 non-zeros: refused, no output touched
    qm = _matrix(rng, 3, 4200, dt, 0.01)
    qm[1, 50:4147] = 1.0
    d = _dev(qm)
    keys, scores, cnts = _dev(np.full((3, 5), 99, np.uint64)), _dev(np.full((3, 5), 9.0, np.float32)), _dev(np.full(3, 77, np.uint32))
    ctx = se.create_context()
    L = _lib()
    assert L.zvec_hip_sparse_search_dense_dev(se._h, ctx._h, _p(d), 3, 4200, 4200, 5, FLT_MAX, None, _p(keys), _p(scores), _p(cnts),
                                              None) == INVALID
    assert L.zvec_hip_sparse_search_dense_dev(se._h, ctx._h, _p(d), 3, 4200, 4199, 5, FLT_MAX, None, _p(keys), _p(scores), _p(cnts),
                                              None) == INVALID
    assert L.zvec_hip_sparse_search_dense_dev(se._h, ctx._h, _p(d), 3, 4200, 4200, 0, FLT_MAX, None, _p(keys), _p(scores), _p(cnts),
                                              None) == INVALID
    ctx.synchronize()
    assert (_host(keys) == 99).all() and (_host(scores) == 9.0).all() and (_host(cnts) == 77).all()


# ---- 6. the inverted lists go out of date -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_device_append_marks_the_inverted_lists_out_of_date(dtype):
    dt = NP[dtype]
    rng = np.random.default_rng([8, DT[dtype]])
    first, second, third = (_matrix(rng, n, 400, dt, 0.05) for n in (50, 30, 20))
    query = G.dense_to_csr(_matrix(rng, 4, 400, dt, 0.1))
    se = _new(dtype)
    se.set_inverted(True)
    assert se.add_batch(*G.dense_to_csr(first)) == 0
    _search(se, query, 8)
    builds = se.inverted_info()["builds"]
    assert builds == 1
    assert _append_dense(se, second) == 0
    assert se.inverted_info()["builds"] == builds                        # (the append itself builds nothing)
    _search(se, query, 8)
    assert se.inverted_info()["builds"] == builds + 1
    assert _append_csr(se, G.dense_to_csr(third)) == 0
    got = _search(se, query, 8)
    _search(se, query, 8)
    assert se.inverted_info()["builds"] == builds + 2                    # once per append, not per search
    fresh = _new(dtype)
    fresh.set_inverted(True)
    assert fresh.add_batch(*G.dense_to_csr(np.concatenate([first, second, third]))) == 0
    assert got == _search(fresh, query, 8)


# ---- 7. ingest_info ---------------------------------------------------------------------------------------------------------------------
def test_ingest_info_tells_the_last_successful_call():
    rng = np.random.default_rng(9)
    se = _new("fp32")
    info = _info(se)
    assert info["route"] == -1 and info["elements"] == 0 and info["slice_cols"] > 0
    m = _matrix(rng, 12, 90, np.float32, 0.2)
    csr = G.dense_to_csr(m)
    assert _append_csr(se, csr) == 0
    assert _info(se)["route"] == 0 and _info(se)["elements"] == csr[1].size and _info(se)["ms"] > 0.0
    assert _append_dense(se, m[:5]) == 0
    assert _info(se)["route"] == 1 and _info(se)["elements"] == int(csr[0][:5].sum())
    L = _lib()
    assert L.zvec_hip_sparse_ingest_info(se._h, None, None, None, None) == 0
    assert L.zvec_hip_sparse_ingest_info(None, None, None, None, None) == INVALID


# ---- 8. the Python wrappers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_wrappers_take_torch_tensors(dtype):
    import torch
    import zvec_amd as zv
    dt = NP[dtype]
    rng = np.random.default_rng([10, DT[dtype]])
    n, dim = 90, 333
    m = _matrix(rng, n, dim, dt, 0.1)
    wide = _dev(np.concatenate([m, np.full((n, 5), 7.0, dt)], axis=1))
    view = wide[:, :dim]                                                 # rows stride(0) = dim + 5 elements apart
    assert view.stride(0) == dim + 5 and not view.is_contiguous()
    counts, idx, val = G.dense_to_csr(m)
    tc, ti, tv = zv.sparse_from_dense(view)
    assert np.array_equal(_host(tc), counts) and np.array_equal(_host(ti), idx) and G.raw(_host(tv)).tobytes() == G.raw(val).tobytes()
    keys = np.arange(n, dtype=np.uint64) + 1000
    a, b, c = _new(dtype), _new(dtype), _new(dtype)
    assert a.add_dense(view, keys=_dev(keys)) == 0
    assert b.add_csr_dev(tc, ti, tv, keys=_dev(keys)) == 0
    assert c.add_batch(counts, idx, val, keys=keys) == 0
    G.assert_same_store(G.read_store(a), G.read_store(c))
    G.assert_same_store(G.read_store(b), G.read_store(c))
    assert np.array_equal(a._all_keys(), keys) and np.array_equal(b._all_keys(), keys)
    qm = _matrix(rng, 6, dim, dt, 0.1)
    k, s, cn = a.search_dense(_dev(qm), 9)
    want = _search(c, G.dense_to_csr(qm), 9)
    assert (_host(k).tobytes(), _host(s).tobytes(), _host(cn).tobytes()) == want
    other = torch.float32 if dtype == "fp16" else torch.float16
    for call in (lambda: a.add_dense(torch.from_numpy(m)), lambda: a.add_dense(view.to(other)),
                 lambda: a.search_dense(torch.from_numpy(qm), 3), lambda: a.search_dense(_dev(qm).to(other), 3),
                 lambda: a.add_csr_dev(tc.cpu(), ti, tv), lambda: a.add_csr_dev(tc, ti, tv.to(other)),
                 lambda: zv.sparse_from_dense(torch.from_numpy(m)), lambda: zv.sparse_from_dense(_dev(qm).to(torch.float64))):
        with pytest.raises(ValueError):
            call()
    assert a.count() == n


# ---- 9. the host entries' results do not move -----------------------------------------------------------------------------------------
def test_host_results_are_the_same_before_and_after_the_device_entries_ran():
    rng = np.random.default_rng(11)
    rows = _matrix(rng, 400, 800, np.float32, 0.05)
    query = G.dense_to_csr(_matrix(rng, 9, 800, np.float32, 0.05))
    host = _new("fp32")
    assert host.add_batch(*G.dense_to_csr(rows)) == 0
    before = _search(host, query, 20)
    other = _new("fp32")
    assert _append_dense(other, rows, 801, 1) == 0 and _append_csr(other, G.dense_to_csr(rows)) == 0
    other.search_dense(_dev(rows[:3]), 5)
    assert _search(host, query, 20) == before


# ---- 10. more work items than one segment of the offset scan holds ---------------------------------------------------------------------
def test_calls_longer_than_one_scan_segment():
    """the offsets are scanned in segments of 2^20 work items, each on top of the 64-bit sum of those before it: a CSR call of more
    rows than that, and a dense call of more (row, slice) items, sampled around the segment boundary against the reference"""
    rng = np.random.default_rng(12)
    n = (1 << 20) + 70
    sample = np.unique(np.concatenate([[0, 1, n - 1], np.arange((1 << 20) - 3, (1 << 20) + 3), rng.integers(0, n, 40)]))
    counts = (np.arange(n) % 3 == 0).astype(np.uint32) * 2
    idx = np.repeat(np.arange(n, dtype=np.uint32) % 1000, counts)
    idx[1::2] += 1 + idx[1::2] % 7                                       # (two ascending indices a row)
    val = (np.arange(idx.size) % 251 + 1).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    se = _new("fp32")
    assert _append_csr(se, (counts, idx, val)) == 0
    assert se.count() == n and se.element_count() == idx.size
    for p in sample:
        i, v = se.get_vector_by_id(int(p))
        assert np.array_equal(i, idx[off[p]:off[p + 1]]) and np.array_equal(v, val[off[p]:off[p + 1]]), p
    bad = idx.copy()
    last = int(np.nonzero(counts)[0][-1])                                # the last row with pairs, behind the boundary, repeats an index
    bad[off[last] + 1] = bad[off[last]]
    assert last > (1 << 20) and _append_csr(se, (counts, bad, val)) == INVALID and se.count() == n
    m = np.zeros((n, 2), np.float32)
    m[::5, 1] = np.arange(0, n, 5) % 97 + 1.0
    m[::7, 0] = -1.0
    de = _new("fp32")
    assert _append_dense(de, m, 3, 1) == 0
    assert de.count() == n and de.element_count() == int((m != 0).sum())
    for p in sample:
        i, v = de.get_vector_by_id(int(p))
        keep = np.nonzero(m[p])[0]
        assert np.array_equal(i, keep.astype(np.uint32)) and np.array_equal(v, m[p, keep]), p

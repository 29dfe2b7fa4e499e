"""Add-with-id on the sparse index from device memory (zvec_hip_sparse_put_dev) on the GPU.  Every case runs twice: on a handle
written through put_dev with the call's arrays as torch tensors on the device, and on a twin written through the host
zvec_hip_sparse_put with the same arrays.  After every call the whole store of both — rows bit for bit through
zvec_hip_sparse_get_vector over every position, keys, holes, counts — equals the Python model of tests/sparse_put_ref.py and each
other, and put_info names the same route for both, the one the case claims.  The cases are those of tests/sparse_put_dev_ref.py,
which tests/test_sparse_put_dev_reference_cpu.py holds to their preconditions; the splice case is sized from put_info's chunk_elems."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_l2_ref as L2  # noqa: E402
import sparse_put_dev_ref as G  # noqa: E402
import sparse_put_ref as M  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

OUT_OF_RANGE, INVALID = -17, -31
FLT_MAX = float(np.finfo(np.float32).max)
DTYPES = ["fp32", "fp16"]
METRICS = ["InnerProductSparse", "SquaredEuclideanSparse"]
NP = M.NP


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _dptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib():
    from zvec_amd import _lib as L
    return L.lib()


def _dev(a, src_off=0):
    """a numpy array as a device tensor of the same bits that starts src_off elements into a larger one"""
    import torch
    a = np.ascontiguousarray(a)
    bits = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    big = torch.full((src_off + a.size + 3,), -1, dtype=getattr(torch, np.dtype(bits).name), device="cuda")
    view = big[src_off:src_off + a.size]
    view.copy_(torch.from_numpy(a.view(bits).copy()))
    assert a.size == 0 or view.data_ptr() == big.data_ptr() + src_off * a.dtype.itemsize      # (an empty view has no address)
    return view


class Twins:
    """a handle fed through put_dev, its twin fed through the host put, and the model of both"""

    def __init__(self, dtype, metric="InnerProductSparse"):
        import zvec_amd as zv
        self.dev = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
        self.host = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
        self.model = M.PutModel(dtype)

    def put_dev(self, ids, counts, idx, val, keys=None, src_off=0, stream=None):
        """the C entry on device copies of the arrays: (status, the tensors, kept alive by the caller)"""
        import torch
        ids, counts = np.asarray(ids, np.uint32), np.asarray(counts, np.uint32)
        t = [_dev(ids), _dev(counts), _dev(idx, src_off), _dev(val, src_off), None if keys is None else _dev(np.asarray(keys, np.uint64))]
        torch.cuda.synchronize()
        rc = _lib().zvec_hip_sparse_put_dev(self.dev._h, _dptr(t[0]), _dptr(t[1]), _dptr(t[2]), _dptr(t[3]), ids.size, idx.size,
                                            _dptr(t[4]), stream)
        return rc

    def check(self):
        a, b = M.read_store(self.dev), M.read_store(self.host)
        M.check_store(a, self.model)
        M.check_store(b, self.model)
        assert a["count"] == b["count"] and a["elements"] == b["elements"] and a["holes"] == b["holes"]
        assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["hole"], b["hole"])
        for (ai, av), (bi, bv) in zip(a["rows"], b["rows"]):
            assert ai.tobytes() == bi.tobytes() and M.raw(av).tobytes() == M.raw(bv).tobytes()

    def step(self, step, check=True):
        L = _lib()
        counts, idx, val = M.pack(step["rows"], self.model.np_dtype)
        if step["kind"] == "append":
            for se in (self.dev, self.host):
                assert L.zvec_hip_sparse_append(se._h, _ptr(counts), _ptr(idx), _ptr(val), counts.size, None) == 0
        else:
            ids = np.asarray(step["ids"], np.uint32)
            keys = None if step["keys"] is None else np.asarray(step["keys"], np.uint64)
            assert self.put_dev(ids, counts, idx, val, keys, step["src_off"]) == 0
            assert L.zvec_hip_sparse_put(self.host._h, _ptr(ids), _ptr(counts), _ptr(idx), _ptr(val), ids.size, _ptr(keys)) == 0
            a, b = self.dev.put_info(), self.host.put_info()
            assert a["route"] == b["route"] == step["route"], (a, b, step["ids"])
            assert a["moved_elems"] == b["moved_elems"] and a["chunk_elems"] == b["chunk_elems"]
        G.apply_step(self.model, step)
        if check:
            self.check()

    def run(self, steps, check=True):
        for s in steps:
            self.step(s, check)
        return self


def _chunk():
    import zvec_amd as zv
    return zv.HipFlatSparseStreamer().put_info()["chunk_elems"]


# ---- 1 .. 5: the routes, the source alignments, keep-last -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_tail_route_holes_and_a_host_append_on_top(dtype):
    t = Twins(dtype).run(G.case_tail(dtype))
    assert t.dev.holes() == len(t.model.holes) > 0 and t.dev.count() == t.model.count() > 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_route(dtype):
    t = Twins(dtype).run(G.case_in_place(dtype))
    assert t.dev.put_info()["route"] == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_splice_route_at_the_chunk_boundaries(dtype):
    chunk = _chunk()
    steps, (a, b, c) = G.case_splice(dtype, chunk)
    t = Twins(dtype)
    t.step(steps[0])
    off = G.offsets(t.model)
    assert off[a + 1] == chunk and off[b + 1] == 2 * chunk - 1 and off[c + 1] == 3 * chunk + 1 and t.dev.element_count() > 3 * chunk
    for s in steps[1:]:
        t.step(s)
        assert t.dev.put_info()["moved_elems"] == t.model.elements()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src_off", [1, 2, 3])
def test_source_views_off_the_word_grid(src_off, dtype):
    Twins(dtype).run(G.case_alignment(dtype, src_off))


@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_last_with_descending_ids(dtype):
    Twins(dtype).run(G.case_keep_last(dtype))


@pytest.mark.parametrize("metric", METRICS)
def test_both_metrics_take_the_same_put(metric):
    Twins("fp16", metric).run(G.case_keep_last("fp16"))


def test_put_dev_on_a_stream_of_the_callers():
    import torch
    t = Twins("fp16")
    steps = G.case_keep_last("fp16")
    s = torch.cuda.Stream()
    for step in steps:
        counts, idx, val = M.pack(step["rows"], t.model.np_dtype)
        ids = np.asarray(step["ids"], np.uint32)
        keys = None if step["keys"] is None else np.asarray(step["keys"], np.uint64)
        assert t.put_dev(ids, counts, idx, val, keys, 1, C.c_void_p(s.cuda_stream)) == 0
        assert _lib().zvec_hip_sparse_put(t.host._h, _ptr(ids), _ptr(counts), _ptr(idx), _ptr(val), ids.size, _ptr(keys)) == 0
        G.apply_step(t.model, step)
        assert t.dev.put_info()["route"] == t.host.put_info()["route"] == step["route"]
        t.check()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_calls_leave_everything_as_it_was(dtype):
    rng = np.random.default_rng(9)
    t = Twins(dtype)
    t.dev.set_inverted(True)
    t.run(G.case_keep_last(dtype)[:2])
    npdt = NP[dtype]
    good = M.random_row(rng, 6, G.VOCAB, npdt)
    q = (np.array([2], np.uint32), good[0][:2].copy(), np.ones(2, npdt))
    _search(t.dev, q, 3)                                                 # the lists are built: a refused call must leave them so
    built = t.dev.inverted_info()
    assert built["builds"] == 1
    unsorted = good[0].copy()
    unsorted[[2, 3]] = unsorted[[3, 2]]
    repeated = good[0].copy()
    repeated[4] = repeated[3]
    two = M.pack([good, good], npdt)
    long_idx, long_val = np.arange(4097, dtype=np.uint32), np.ones(4097, npdt)
    L = _lib()

    def null_ids():
        c, i, v = _dev(np.array([6], np.uint32)), _dev(good[0]), _dev(good[1])
        return L.zvec_hip_sparse_put_dev(t.dev._h, None, _dptr(c), _dptr(i), _dptr(v), 1, 6, None, None)

    def wrong_sum():
        d, c, i, v = _dev(np.array([1, 2], np.uint32)), _dev(two[0]), _dev(two[1]), _dev(two[2])
        return L.zvec_hip_sparse_put_dev(t.dev._h, _dptr(d), _dptr(c), _dptr(i), _dptr(v), 2, 11, None, None)

    cases = [
        ("a run that does not ascend", INVALID, lambda: t.put_dev([1, 2], two[0], np.concatenate([good[0], unsorted]), two[2])),
        ("a repeated index", INVALID, lambda: t.put_dev([1, 2], two[0], np.concatenate([good[0], repeated]), two[2])),
        ("a row of 4097 pairs", INVALID, lambda: t.put_dev([1], [4097], long_idx, long_val)),
        ("counts that do not sum to elements", INVALID, wrong_sum),
        ("id 2^32 - 1", OUT_OF_RANGE, lambda: t.put_dev([1, 0xffffffff], two[0], two[1], two[2])),
        ("more rows than the store takes", OUT_OF_RANGE, lambda: t.put_dev([0xfffffffe], [6], good[0], good[1])),
        ("NULL d_ids", INVALID, null_ids),
    ]
    info = t.dev.put_info()
    for what, code, fn in cases:
        assert fn() == code, what
        t.check()
        now = t.dev.put_info()
        assert (now["route"], now["moved_elems"], now["ms"]) == (info["route"], info["moved_elems"], info["ms"]), what
        assert t.dev.inverted_info() == built, what
    _search(t.dev, q, 3)
    assert t.dev.inverted_info() == built                                # (still current: no search had to rebuild them)
    assert L.zvec_hip_sparse_put_dev(None, None, None, None, None, 0, 0, None, None) == INVALID
    assert L.zvec_hip_sparse_put_dev(t.dev._h, None, None, None, None, 0, 0, None, None) == 0      # n == 0
    assert t.dev.put_info()["ms"] == info["ms"]
    t.check()
    # the handle still takes a put afterwards
    t.step(G.put([1, len(G.BASE)], [good, good], 2))


# ---- 7. searches after puts -------------------------------------------------------------------------------------------------------
def _search(se, queries, k):
    c, i, v = queries
    nq = len(c)
    keys, scores, counts = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    rc = _lib().zvec_hip_sparse_search(se._h, None, _ptr(c), _ptr(i), _ptr(v), nq, k, FLT_MAX, None, _ptr(keys), _ptr(scores), _ptr(counts))
    assert rc == 0, rc
    return keys, scores, counts


def _check_lists(metric, got, model, queries, k):
    rows = model.batch()
    n = model.count()
    admissible = ~model.hole_mask()
    key_of_row = np.array([model.keys[r] if r not in model.holes else (1 << 63) + r for r in range(n)], np.uint64)     # (distinct)
    if metric == "InnerProductSparse":
        ref, A = R.sparse_reference(rows, queries)
        R.check_sparse_lists(*got, ref, A, R.shared_counts(rows, queries), k, None, admissible, key_of_row)
    else:
        L2.check_sparse_l2_lists(*got, L2.sparse_l2_reference(rows, queries), k, None, admissible, key_of_row)


def _same_answer(a, b):
    assert np.array_equal(a[2], b[2])
    for q in range(len(a[2])):
        c = int(a[2][q])
        assert np.array_equal(a[0][q, :c], b[0][q, :c]) and a[1][q, :c].tobytes() == b[1][q, :c].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_search_after_a_mixed_sequence(metric, dtype):
    steps, queries = G.case_search(dtype, metric)
    t = Twins(dtype, metric).run(steps, check=False)
    t.check()
    for k in (10, 400):
        got, want = _search(t.dev, queries, k), _search(t.host, queries, k)
        _same_answer(got, want)
        _check_lists(metric, got, t.model, queries, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inverted_lists_are_rebuilt_after_a_put_dev(dtype):
    metric = "InnerProductSparse"
    steps, queries = G.case_search(dtype, metric)
    t = Twins(dtype, metric)
    t.dev.set_inverted(True)
    t.host.set_inverted(True)
    t.run(steps[:2], check=False)
    _same_answer(_search(t.dev, queries, 10), _search(t.host, queries, 10))
    builds = t.dev.inverted_info()["builds"]
    assert builds == 1
    for s in steps[2:]:
        t.step(s, check=False)
        assert t.dev.inverted_info()["builds"] == builds                     # (a put only marks the lists out of date)
        got = _search(t.dev, queries, 60)
        builds += 1
        assert t.dev.inverted_info()["builds"] == builds
        _same_answer(got, _search(t.host, queries, 60))
        _check_lists(metric, got, t.model, queries, 60)
    t.check()


# ---- 8. through Python ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_index_put_dev_ends_in_the_store_of_index_put(dtype):
    import torch
    import zvec_amd as zv
    a, b = zv.HipFlatSparseStreamer(dtype=dtype), zv.HipFlatSparseStreamer(dtype=dtype)
    model = M.PutModel(dtype)
    tdt = torch.float16 if dtype == "fp16" else torch.float32
    for step in G.case_keep_last(dtype) + G.case_tail(dtype)[-1:]:
        counts, idx, val = M.pack(step["rows"], model.np_dtype)
        ids = np.asarray(step["ids"], np.uint32)
        keys = None if step["keys"] is None else np.asarray(step["keys"], np.uint64)
        dev = [torch.from_numpy(x.astype(np.int32)).cuda() for x in (ids, counts, idx)]
        rc = a.put_dev(dev[0], dev[1], dev[2], torch.from_numpy(val).cuda().to(tdt),
                       None if keys is None else torch.from_numpy(keys.astype(np.int64)).cuda())
        assert rc == 0 and b.add_with_id_batch(ids, counts, idx, val, keys) == 0
        G.apply_step(model, step)
        assert a.put_info()["route"] == b.put_info()["route"]
        M.check_store(M.read_store(a), model)
        M.check_store(M.read_store(b), model)
        assert np.array_equal(a._all_keys(), b._all_keys()) and np.array_equal(a._all_keys(), np.array(model.keys, np.uint64))
    with pytest.raises(ValueError):
        a.put_dev(torch.zeros(1, dtype=torch.int32), dev[1][:1], dev[2][:0], torch.zeros(0, dtype=tdt).cuda())      # a CPU tensor
    with pytest.raises(ValueError):
        a.put_dev(dev[0], dev[1], dev[2], torch.zeros(dev[2].numel(), dtype=torch.float64).cuda())                   # a wrong dtype
    s = torch.cuda.Stream()
    one = M.random_row(np.random.default_rng(3), 5, G.VOCAB, NP[dtype])
    args = [torch.tensor([2], dtype=torch.int32).cuda(), torch.tensor([5], dtype=torch.int32).cuda(),
            torch.from_numpy(one[0].astype(np.int32)).cuda(), torch.from_numpy(one[1]).cuda()]
    torch.cuda.synchronize()
    assert a.put_dev(*args, stream=s) == 0 and b.add_with_id_impl(2, one[0], one[1]) == 0
    M.apply_put(model, [2], [5], one[0], one[1])
    M.check_store(M.read_store(a), model)
    M.check_store(M.read_store(b), model)

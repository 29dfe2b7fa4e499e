"""Add-with-id on the sparse index on the GPU (zvec_hip_sparse_put, zvec_hip_sparse_holes, zvec_hip_sparse_put_info) against the
Python model of tests/sparse_put_ref.py: after every put the whole store — rows bit for bit through get_vector, keys, holes, counts —
equals the model, and put_info names the route the case was built for (0 tail, 1 in place, 2 splice; the splice cases are sized
from put_info's chunk_elems).  Searches over a store built by puts are held to fp64 over the model's rows and, bit for bit, to a
second handle filled by one append.  Both value types throughout."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_l2_ref as L2  # noqa: E402
import sparse_put_ref as M  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_OF_RANGE, INVALID = -17, -31
FLT_MAX = float(np.finfo(np.float32).max)
DTYPES = ["fp32", "fp16"]
NP = M.NP
VOCAB = 6000


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _lib():
    from zvec_amd import _lib as L
    return L.lib()


def _new(dtype, metric="InnerProductSparse"):
    import zvec_amd as zv
    return zv.HipFlatSparseStreamer(dtype=dtype, metric=metric), M.PutModel(dtype)


def _rows(rng, lengths, dtype, vocab=VOCAB):
    """random rows; those of the small vocabularies are searched and carry no denormals (the fp64 bands assume products that do
    not underflow), the others are only moved and read back, special bit patterns included"""
    return [M.random_row(rng, c, vocab, NP[dtype], specials=vocab == VOCAB) for c in lengths]


def _put(se, model, ids, rows, keys=None, route=None, check=True):
    """one put on the handle and on the model; the route it took; the whole store against the model"""
    counts, idx, val = M.pack(rows, model.np_dtype)
    k = None if keys is None else np.asarray(keys, np.uint64)
    assert se.add_with_id_batch(ids, counts, idx, val, k) == 0
    M.apply_put(model, ids, counts, idx, val, keys)
    info = se.put_info()
    if route is not None:
        assert info["route"] == route, (info, ids)
    if check:
        M.check_store(M.read_store(se), model)
        assert np.array_equal(se._all_keys(), np.array(model.keys, np.uint64))
    return info


def _filled(dtype, lengths, seed, metric="InnerProductSparse"):
    """a handle and its model holding rows of the given lengths at ids 0 .. n - 1 (one tail put)"""
    rng = np.random.default_rng([seed, len(lengths), int(dtype == "fp16")])
    se, model = _new(dtype, metric)
    _put(se, model, np.arange(len(lengths)), _rows(rng, lengths, dtype), route=0)
    return se, model, rng


def _chunk():
    import zvec_amd as zv
    return zv.HipFlatSparseStreamer().put_info()["chunk_elems"]


# ---- 1. tail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_put_of_the_next_ids_equals_an_append(dtype):
    import zvec_amd as zv
    rng = np.random.default_rng(1)
    lengths = [5, 0, 17, 1, 4096, 3, 64, 65, 0, 9]
    rows = _rows(rng, lengths, dtype)
    se, model = _new(dtype)
    assert se.put_info()["route"] == -1 and se.put_info()["chunk_elems"] > 0
    _put(se, model, [0, 1, 2, 3], rows[:4], route=0)
    info = _put(se, model, [4, 5, 6, 7, 8, 9], rows[4:], route=0)
    assert info["moved_elems"] == sum(lengths[4:])
    ap = zv.HipFlatSparseStreamer(dtype=dtype)
    assert ap.add_batch(*M.pack(rows, NP[dtype])) == 0
    assert ap.count() == se.count() == 10 and ap.element_count() == se.element_count() == sum(lengths) and se.holes() == 0
    for r in range(10):
        a, b = ap.get_vector_by_id(r), se.get_vector_by_id(r)
        assert np.array_equal(a[0], b[0]) and M.raw(a[1]).tobytes() == M.raw(b[1]).tobytes()
    assert se.add_with_id_batch([], [], [], []) == 0 and se.count() == 10           # n == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaps_become_holes_that_no_search_returns(dtype):
    rng = np.random.default_rng(2)
    se, model = _new(dtype)
    _put(se, model, [3], _rows(rng, [4], dtype), route=0)                            # a gap in front of the first row
    assert se.holes() == 3
    _put(se, model, [4, 9, 10, 70, 200], _rows(rng, [2, 0, 5, 7, 1], dtype), keys=[104, 109, 110, 170, 1200], route=0)
    assert se.holes() == 3 + 4 + 59 + 129 and se.count() == 201
    for r in (0, 5, 69, 199):
        i, v = se.get_vector_by_id(r)
        assert i.size == 0 and v.size == 0
    # a query that shares no index with any row scores 0 everywhere: the zero ties would admit the holes if they were not excluded
    ctx = se.create_context()
    ctx.set_topk(201)
    q = (np.array([2], np.uint32), np.array([VOCAB + 5, VOCAB + 9], np.uint32), np.ones(2, NP[dtype]))
    assert se.search_impl(*q, 1, ctx) == 0
    live = 201 - se.holes()
    assert int(ctx.counts[0]) == live == 6
    got = sorted(int(k) for k in ctx.keys[0, :live])
    assert got == sorted(k for k in model.keys if k != M.INVALID_KEY) and M.INVALID_KEY not in got
    assert not ctx.scores[0, :live].any()


# ---- 2. in place ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_length_overwrites_stay_in_place(dtype):
    lengths = [7, 0, 33, 1, 64, 4096, 2, 65, 12, 5]
    se, model, rng = _filled(dtype, lengths, 3)
    before = model.copy()
    ids = [7, 2, 5, 1, 9]
    info = _put(se, model, ids, _rows(rng, [lengths[i] for i in ids], dtype), keys=[507, 502, 505, 501, 509], route=1)
    assert info["moved_elems"] == sum(lengths[i] for i in ids)
    got = M.read_store(se)                              # every other row and key as the handle held it before, bit for bit
    for r in range(len(lengths)):
        if r not in ids:
            assert int(got["keys"][r]) == before.keys[r] and np.array_equal(got["rows"][r][0], before.rows[r][0])
            assert M.raw(got["rows"][r][1]).tobytes() == M.raw(before.rows[r][1]).tobytes()
    # equal lengths with rows behind the old end in the same call: still in place, the tail rows appended
    info = _put(se, model, [4, 10, 12], _rows(rng, [64, 3, 8], dtype), route=1)
    assert info["moved_elems"] == 64 + 3 + 8 and se.holes() == 1
    # an empty row over a hole keeps its length too
    _put(se, model, [11], _rows(rng, [0], dtype), route=1)
    assert se.holes() == 0


# ---- 3. splice ------------------------------------------------------------------------------------------------------------------
BASE = [5, 9, 0, 7, 12, 3, 30, 1]


def _splice_steps(name, n):
    """(ids, lengths) of every put of a scenario over a store of the BASE lengths; each has to take the splice"""
    return {
        "shrink and grow": [([1], [4]), ([1], [20]), ([6], [29])],
        "to empty and from empty": [([3], [0]), ([3], [6]), ([2], [4])],
        "first and last row": [([0], [6]), ([n - 1], [3]), ([0, n - 1], [0, 0]), ([0, n - 1], [2, 2])],
        "two adjacent rows": [([3, 4], [8, 11]), ([4, 5, 6], [1, 1, 1]), ([0, 1], [1, 1])],
        "the same id twice": [([4, 4], [3, 11]), ([2, 5, 2], [6, 3, 2])],
        "mixed with tail rows and a gap": [([1, n + 3, n, 2, n + 3], [2, 5, 4, 3, 6]), ([n + 1, 0], [2, 9])],
        "lengths 0, 1 and 4096": [([1], [4096]), ([1], [1]), ([5], [4096]), ([1, 5], [0, 1]), ([1], [1])],
        "odd and even shifts": [([1], [10]), ([1], [9]), ([1], [12]), ([0], [6]), ([0, 3], [5, 10])],
    }[name]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["shrink and grow", "to empty and from empty", "first and last row", "two adjacent rows",
                                  "the same id twice", "mixed with tail rows and a gap", "lengths 0, 1 and 4096", "odd and even shifts"])
def test_splice(name, dtype):
    se, model, rng = _filled(dtype, BASE, 4)
    for ids, lengths in _splice_steps(name, len(BASE)):
        before = model.elements()
        info = _put(se, model, ids, _rows(rng, lengths, dtype), route=2)
        assert info["moved_elems"] == model.elements()
        if name == "odd and even shifts" and len(ids) == 1:
            assert abs(model.elements() - before) in (1, 3)          # rows behind it move by +1, -1, +3, +1 elements


@pytest.mark.parametrize("dtype", DTYPES)
def test_splice_fills_a_hole(dtype):
    se, model, rng = _filled(dtype, BASE, 5)
    n = len(BASE)
    _put(se, model, [n + 2], _rows(rng, [4], dtype), route=0)
    assert se.holes() == 2
    _put(se, model, [n], _rows(rng, [5], dtype), route=2)
    assert se.holes() == 1
    _put(se, model, [n + 1, 2], _rows(rng, [3, 1], dtype), keys=[900, 901], route=2)
    assert se.holes() == 0 and se.element_count() == model.elements()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("j", [1, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_splice_at_the_chunk_boundaries(j, d, dtype):
    """a store of chunk_elems * j + d elements in rows of 100; the touched rows lie across the boundaries between the chunks (and
    at the end of the last one) and trade elements, so the store has that many elements before and after"""
    chunk = _chunk()
    E = chunk * j + d
    k = E // 100 - 1
    lengths = [100] * k + [E - 100 * k]
    off = np.concatenate([[0], np.cumsum(lengths)])
    se, model, rng = _filled(dtype, lengths, 6)
    assert se.element_count() == E
    last = len(lengths) - 1
    across = [r for r in range(last) if off[r] // chunk != (off[r + 1] - 1) // chunk]      # rows that span a chunk boundary
    if j == 1:
        assert across == [] and (d < 1 or (off[last] < chunk < off[last + 1]))
        steps = [([0, last], [101, lengths[last] - 1]), ([last, 0], [lengths[last] + 2, 98])]
    else:
        assert len(across) == 2
        a, b = across
        steps = [([a, b, last], [101, 102, lengths[last] - 3]), ([b, a], [99, 104]), ([last, a], [lengths[last] + 2, 99])]
    for ids, new in steps:
        _put(se, model, ids, _rows(rng, new, dtype), route=2)
        assert model.elements() in (E, E + 1, E + 3) and se.put_info()["moved_elems"] == model.elements()


# ---- 3a. what both routes that overwrite share: the pieces kernel and the keep-last rule ------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [255, 256, 257])
@pytest.mark.parametrize("route", [1, 2])
def test_overwritten_rows_at_the_block_edge_of_the_pieces_kernel(route, m, dtype):
    """sparse_put_pieces_kernel runs m + 1 threads in blocks of 256 and thread m writes the closing pieces: m = 255 fills one block
    exactly, 256 and 257 put the closing thread first and second in a block of its own.  A store of 300 rows of one or two pairs;
    the call overwrites m of them in any order and brings two tail rows with a gap between; in place with every length kept, a
    splice with every second overwritten row one pair longer"""
    lengths = [1 + r % 2 for r in range(300)]
    se, model, rng = _filled(dtype, lengths, 12)
    over = rng.permutation(300)[:m]
    longer = set(sorted(int(i) for i in over)[1::2]) if route == 2 else set()
    ids = [int(i) for i in over] + [302, 300]
    new = [lengths[i] + (i in longer) for i in ids[:m]] + [3, 2]
    info = _put(se, model, ids, _rows(rng, new, dtype), route=route)
    assert se.holes() == 1 and se.count() == 303
    assert info["moved_elems"] == (sum(new) if route == 1 else model.elements())
    assert model.elements() == sum(lengths) + len(longer) + 5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", [1, 2])
def test_ids_out_of_order_and_twice_keep_the_last_row(route, dtype):
    """[6, 2, 6, 9, 2] on a store of 8 rows: the third and the fifth row of the call are the ones that stay, with their keys; once
    they are as long as the stored rows (in place, whatever the first and the second row held), once not (splice)"""
    base = [5, 9, 4, 7, 12, 3, 30, 1]
    se, model, rng = _filled(dtype, base, 13)
    ids = [6, 2, 6, 9, 2]
    new = [11, 6, 30, 2, 4] if route == 1 else [30, 4, 29, 2, 6]
    info = _put(se, model, ids, _rows(rng, new, dtype), keys=[601, 201, 602, 901, 202], route=route)
    assert [model.keys[i] for i in (2, 6, 9)] == [202, 602, 901] and se.holes() == 1
    assert info["moved_elems"] == (30 + 4 + 2 if route == 1 else model.elements())
    assert model.elements() == sum(base) + 2 + (0 if route == 1 else 1)


# ---- 4. searches after puts -----------------------------------------------------------------------------------------------------
def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


_BUILT = {}


def _built_by_puts(dtype, metric):
    """(handle built by a sequence of puts, its model, a second handle filled by ONE append of the model's final rows with holes as
    empty rows, the queries), shared by the tests below: nothing there changes them"""
    key = (dtype, metric)
    if key not in _BUILT:
        import zvec_amd as zv
        rng = np.random.default_rng([7, int(dtype == "fp16"), int(metric == "InnerProductSparse")])
        vocab = 60
        se, model = _new(dtype, metric)
        lens = rng.choice([0, 1, 8, 20], 300)
        _put(se, model, np.arange(300), _rows(rng, lens, dtype, vocab), route=0, check=False)
        _put(se, model, [320, 305, 340], _rows(rng, [9, 4, 12], dtype, vocab), keys=[9320, 9305, 9340], route=0, check=False)     # gaps
        ids = rng.choice(300, 40, replace=False)
        _put(se, model, ids, _rows(rng, rng.choice([0, 3, 25], 40), dtype, vocab), route=2, check=False)                        # splice
        ids = [int(i) for i in ids[:10]]
        _put(se, model, ids, _rows(rng, [model.rows[i][0].size for i in ids], dtype, vocab), route=1, check=False)              # in place
        _put(se, model, [310, 7, 345, 7], _rows(rng, [6, 2, 3, 30], dtype, vocab), route=2, check=False)                        # hole, tail, twice
        M.check_store(M.read_store(se), model)
        assert se.holes() == len(model.holes) > 20
        ap = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
        assert ap.add_batch(*model.batch(), np.array(model.keys, np.uint64)) == 0
        ql = rng.choice([0, 1, 10, 40], 9)
        queries = R.random_runs(rng, ql, vocab)
        queries = (queries[0], queries[1], queries[2].astype(NP[dtype]))
        _BUILT[key] = (se, model, ap, queries)
    return _BUILT[key]


def _search(se, queries, k, exclude=None, threshold=FLT_MAX):
    c, i, v = queries
    nq = len(c)
    keys, scores, counts = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    rc = _lib().zvec_hip_sparse_search(se._h, None, _ptr(c), _ptr(i), _ptr(v), nq, k, threshold, _ptr(exclude), _ptr(keys), _ptr(scores),
                                       _ptr(counts))
    assert rc == 0, rc
    return keys, scores, counts


def _check_lists(metric, got, model, queries, k, admissible):
    rows = model.batch()
    n = model.count()
    key_of_row = np.array([model.keys[r] if r not in model.holes else (1 << 63) + r for r in range(n)], np.uint64)     # (distinct)
    if metric == "InnerProductSparse":
        ref, A = R.sparse_reference(rows, queries)
        R.check_sparse_lists(*got, ref, A, R.shared_counts(rows, queries), k, None, admissible, key_of_row)
    else:
        L2.check_sparse_l2_lists(*got, L2.sparse_l2_reference(rows, queries), k, None, admissible, key_of_row)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", ["InnerProductSparse", "SquaredEuclideanSparse"])
@pytest.mark.parametrize("k", [10, 400])          # the fused lists, and the dense-score route (k beyond the rows)
def test_search_after_puts_against_fp64(metric, k, dtype):
    se, model, ap, queries = _built_by_puts(dtype, metric)
    n = model.count()
    holes = model.hole_mask()
    for mask in (None, np.arange(n) % 3 == 1):
        ex = None if mask is None else _words_of(mask)
        got = _search(se, queries, k, ex)
        _check_lists(metric, got, model, queries, k, ~holes if mask is None else ~holes & ~mask)
        # the appended twin, searched with the hole bits (OR the caller's) as its exclude set: the same score bits
        want = _search(ap, queries, k, _words_of(holes if mask is None else holes | mask))
        assert np.array_equal(got[2], want[2])
        for q in range(len(queries[0])):
            c = int(got[2][q])
            assert got[1][q, :c].tobytes() == want[1][q, :c].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", ["InnerProductSparse", "SquaredEuclideanSparse"])
def test_every_other_entry_equals_the_appended_twin(metric, dtype):
    import torch
    se, model, ap, queries = _built_by_puts(dtype, metric)
    L = _lib()
    n = model.count()
    holes = model.hole_mask()
    c, i, v = queries
    nq, k = len(c), 12
    mask = np.arange(n) % 4 == 2
    for caller in (None, mask):
        ex_put = None if caller is None else _words_of(caller)
        ex_app = _words_of(holes if caller is None else holes | caller)

        # the device-pointer form
        def dev(h, ex):
            td = torch.device("cuda:0")
            d_i = torch.from_numpy(i.view(np.int32).copy()).to(td)
            d_v = torch.from_numpy(M.raw(v).view(np.int16 if v.dtype.itemsize == 2 else np.int32).copy()).to(td)
            d_ex = None if ex is None else torch.from_numpy(ex.view(np.int64).copy()).to(td)
            ok, os_, oc = (torch.zeros(nq * k, dtype=torch.int64, device=td), torch.zeros(nq * k, dtype=torch.float32, device=td),
                           torch.zeros(nq, dtype=torch.int32, device=td))
            ctx = h.create_context()
            ts = torch.cuda.Stream(device=td)
            ts.wait_stream(torch.cuda.current_stream(td))
            rc = h.search_dev(c, d_i.data_ptr(), d_v.data_ptr(), nq, k, ok.data_ptr(), os_.data_ptr(), oc.data_ptr(), ctx,
                              d_exclude=None if d_ex is None else d_ex.data_ptr(), stream=ts.cuda_stream)
            assert rc == 0
            ts.synchronize()
            return os_.cpu().numpy().reshape(nq, k), oc.cpu().numpy()
        (s1, c1), (s2, c2) = dev(se, ex_put), dev(ap, ex_app)
        assert np.array_equal(c1, c2) and all(s1[q, :c1[q]].tobytes() == s2[q, :c1[q]].tobytes() for q in range(nq))
        got = _search(se, queries, k, ex_put)
        assert np.array_equal(got[2].astype(np.int64), c1.astype(np.int64))
        assert all(got[1][q, :c1[q]].tobytes() == s1[q, :c1[q]].tobytes() for q in range(nq))

        # listed rows: every query against positions that include holes, a position twice and one beyond the rows
        lists = [np.concatenate([np.arange(q, n, 5), [3, 3, n + 4]]).astype(np.uint32) for q in range(nq)]
        ids = np.concatenate(lists).astype(np.uint32)
        offs = np.zeros(nq + 1, np.uint32)
        offs[1:] = np.cumsum([len(a) for a in lists])
        res = []
        for h, ex in ((se, ex_put), (ap, ex_app)):
            keys, scores, counts = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
            assert L.zvec_hip_sparse_search_by_ids(h._h, None, _ptr(c), _ptr(i), _ptr(v), nq, _ptr(ids), _ptr(offs), k, FLT_MAX, _ptr(ex),
                                                   _ptr(keys), _ptr(scores), _ptr(counts)) == 0
            res.append((keys, scores, counts))
        assert np.array_equal(res[0][2], res[1][2])
        for q in range(nq):
            cq = int(res[0][2][q])
            assert res[0][1][q, :cq].tobytes() == res[1][1][q, :cq].tobytes() and np.array_equal(res[0][0][q, :cq], res[1][0][q, :cq])
            assert M.INVALID_KEY not in [int(x) for x in res[0][0][q, :cq]]

        # group-by, both kinds
        gof = (np.arange(n) % 7).astype(np.uint32)
        gnum, gk = 4, 3
        for listed in (False, True):
            outs = []
            for h, ex in ((se, ex_put), (ap, ex_app)):
                out = (np.zeros((nq, gnum), np.uint32), np.zeros(nq, np.uint32), np.zeros((nq, gnum, gk), np.uint64),
                       np.zeros((nq, gnum, gk), np.float32), np.zeros((nq, gnum), np.uint32))
                if listed:
                    rc = L.zvec_hip_sparse_search_grouped_by_ids(h._h, None, _ptr(c), _ptr(i), _ptr(v), nq, _ptr(ids), _ptr(offs), _ptr(gof), 7,
                                                                 gnum, gk, FLT_MAX, _ptr(ex), *[_ptr(a) for a in out])
                else:
                    rc = L.zvec_hip_sparse_search_grouped(h._h, None, _ptr(c), _ptr(i), _ptr(v), nq, _ptr(gof), 7, gnum, gk, FLT_MAX, _ptr(ex),
                                                          *[_ptr(a) for a in out])
                assert rc == 0
                outs.append(out)
            a, b = outs
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]) and np.array_equal(a[0], b[0])
            for q in range(nq):
                for gi in range(int(a[1][q])):
                    cg = int(a[4][q, gi])
                    assert a[3][q, gi, :cg].tobytes() == b[3][q, gi, :cg].tobytes() and np.array_equal(a[2][q, gi, :cg], b[2][q, gi, :cg])
                    assert M.INVALID_KEY not in [int(x) for x in a[2][q, gi, :cg]]

    # batch_distance: a hole scores +inf, every other position what the twin scores
    qo = R.offsets(c)
    q = int(np.argmax(c))
    pos = np.concatenate([np.arange(n), [n + 1]]).astype(np.uint32)
    d_put = se.batch_distance(i[qo[q]:qo[q + 1]], v[qo[q]:qo[q + 1]], pos)
    d_app = ap.batch_distance(i[qo[q]:qo[q + 1]], v[qo[q]:qo[q + 1]], pos)
    assert np.all(np.isposinf(d_put[:n][holes])) and np.isposinf(d_put[n])
    assert d_put[:n][~holes].tobytes() == d_app[:n][~holes].tobytes() and np.all(np.isfinite(d_put[:n][~holes]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_inverted_lists_follow_a_put(dtype):
    rng = np.random.default_rng(8)
    se, model = _new(dtype)
    se.set_inverted(True)
    vocab = 40
    _put(se, model, np.arange(50), _rows(rng, rng.choice([0, 2, 9], 50), dtype, vocab), route=0, check=False)
    queries = R.random_runs(rng, [6, 0, 12], vocab)
    queries = (queries[0], queries[1], queries[2].astype(NP[dtype]))
    _search(se, queries, 5)
    builds = se.inverted_info()["builds"]
    assert builds == 1
    # row 11 gives up its pairs for two with indices nobody else holds; a gap follows
    new = (np.array([vocab + 3, vocab + 8], np.uint32), np.array([0.5, -0.25], NP[dtype]))
    _put(se, model, [11, 53], [new, M.random_row(rng, 4, vocab, NP[dtype], specials=False)], route=2 if model.rows[11][0].size != 2 else 1)
    assert se.inverted_info()["builds"] == builds                       # (a put only marks the lists out of date)
    got = _search(se, queries, 60)
    assert se.inverted_info()["builds"] == builds + 1
    _check_lists("InnerProductSparse", got, model, queries, 60, ~model.hole_mask())
    terms, list_off, ppos, pval = se.inverted_export()
    assert se.inverted_info()["builds"] == builds + 1
    counts, idx, val = model.batch()
    assert ppos.size == idx.size == se.element_count()
    row_of = np.repeat(np.arange(model.count()), counts.astype(np.int64))
    for t in range(terms.size):
        rows_t = ppos[int(list_off[t]):int(list_off[t + 1])]
        assert np.array_equal(rows_t, row_of[idx == terms[t]])           # the postings of a term: exactly the rows that hold it now
    at = {int(t): j for j, t in enumerate(terms)}
    assert ppos[int(list_off[at[vocab + 3]]):int(list_off[at[vocab + 3] + 1])].tolist() == [11]
    assert not np.any(np.isin(ppos, sorted(model.holes)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", ["InnerProductSparse", "SquaredEuclideanSparse"])
def test_append_to_a_handle_that_has_holes(metric, dtype):
    """a put with a gap on a small store, then appends to many times its row count (past the words the hole bits' device copy was
    made with, slack included): every search reads hole bits for all rows, so the copy has to follow the appends"""
    import zvec_amd as zv
    rng = np.random.default_rng([11, int(dtype == "fp16"), int(metric == "InnerProductSparse")])
    vocab = 60
    se, model = _new(dtype, metric)
    _put(se, model, [0, 1, 2, 9], _rows(rng, [5, 0, 8, 3], dtype, vocab), route=0)
    assert se.holes() == 6
    for n_more in (40, 6000):                            # 10 rows -> 50 -> 6050: the copy was made for 2 words plus its slack
        rows = _rows(rng, rng.choice([0, 1, 8, 20], n_more), dtype, vocab)
        counts, idx, val = M.pack(rows, NP[dtype])
        n0 = model.count()
        assert se.add_batch(counts, idx, val) == 0
        M.apply_put(model, np.arange(n0, n0 + n_more), counts, idx, val)
    n = model.count()
    _put(se, model, [n + 10, 4], _rows(rng, [7, 2], dtype, vocab), route=2, check=False)    # and a put behind the appends
    n = model.count()
    assert se.count() == n == 6061 and se.holes() == len(model.holes) == 5 + 10
    M.check_store(M.read_store(se), model)
    ap = zv.HipFlatSparseStreamer(dtype=dtype, metric=metric)
    assert ap.add_batch(*model.batch(), np.array(model.keys, np.uint64)) == 0
    queries = R.random_runs(rng, [0, 1, 10, 40, 10], vocab)
    queries = (queries[0], queries[1], queries[2].astype(NP[dtype]))
    holes = model.hole_mask()
    for k in (10, 400):
        for mask in (None, np.arange(n) % 3 == 1):
            got = _search(se, queries, k, None if mask is None else _words_of(mask))
            _check_lists(metric, got, model, queries, k, ~holes if mask is None else ~holes & ~mask)
            want = _search(ap, queries, k, _words_of(holes if mask is None else holes | mask))
            assert np.array_equal(got[2], want[2])
            for q in range(len(queries[0])):
                c = int(got[2][q])
                assert got[1][q, :c].tobytes() == want[1][q, :c].tobytes()
    d = se.batch_distance(queries[1][:1], queries[2][:1], np.arange(n, dtype=np.uint32))
    assert np.all(np.isposinf(d[holes])) and np.all(np.isfinite(d[~holes]))


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_calls_leave_the_store_as_it_was(dtype):
    se, model, rng = _filled(dtype, BASE, 9)
    _put(se, model, [len(BASE) + 2], _rows(rng, [3], dtype), route=0)
    L = _lib()
    npdt = NP[dtype]
    good = M.random_row(rng, 6, VOCAB, npdt)

    def call(ids, counts, idx, val):
        ids = None if ids is None else np.asarray(ids, np.uint32)
        counts = np.asarray(counts, np.uint32)
        return L.zvec_hip_sparse_put(se._h, _ptr(ids), _ptr(counts), _ptr(idx), _ptr(val), len(counts), None)

    unsorted = good[0].copy()
    unsorted[[2, 3]] = unsorted[[3, 2]]
    repeated = good[0].copy()
    repeated[4] = repeated[3]
    long_idx, long_val = np.arange(4097, dtype=np.uint32), np.ones(4097, npdt)
    two = M.pack([good, good], npdt)
    cases = [
        ("an unsorted run", INVALID, lambda: call([1, 2], two[0], np.concatenate([good[0], unsorted]), two[2])),
        ("a repeated index", INVALID, lambda: call([1, 2], two[0], np.concatenate([good[0], repeated]), two[2])),
        ("a run of 4097 pairs", INVALID, lambda: call([1], [4097], long_idx, long_val)),
        ("NULL indices with pairs present", INVALID, lambda: call([1], [6], None, good[1])),
        ("NULL values with pairs present", INVALID, lambda: call([1], [6], good[0], None)),
        ("id 2^32 - 1", OUT_OF_RANGE, lambda: call([1, 0xffffffff], two[0], two[1], two[2])),
        ("more rows than the store takes", OUT_OF_RANGE, lambda: call([0xfffffffe], [6], good[0], good[1])),
        ("NULL ids", INVALID, lambda: call(None, [6], good[0], good[1])),
    ]
    info = se.put_info()
    for what, code, fn in cases:
        assert fn() == code, what
        M.check_store(M.read_store(se), model)
        assert se.put_info()["route"] == info["route"] and se.put_info()["moved_elems"] == info["moved_elems"], what
    # the handle still takes a put afterwards
    _put(se, model, [1, len(BASE)], [good, good], route=2)


# ---- 7. the C example -----------------------------------------------------------------------------------------------------------
def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sparse_put")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "sparse_put.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-lm", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        text = out.stdout.decode()
        assert out.returncode == 0, text
        assert "check passed" in text and "holes 2" in text and "route of the last put 2" in text

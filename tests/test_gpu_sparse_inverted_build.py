"""The device build of a sparse index's term-major twin (option "sparse_inverted_build" = 1, zvk_sparse_invb.hip.h) against the host
build (option at 0) and the numpy model of tests/sparse_inv_build_ref.py, bit for bit, through zvec_hip_sparse_inverted_export and
zvec_hip_sparse_inverted_build_info.  tests/test_sparse_inv_build_reference_cpu.py checks the model against a model of the radix
scheme on the same cases.  B = block_elems (elements one work-group of the scatter handles), W = 64 lanes."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_inv_build_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, OUT_OF_RANGE, INVALID = -12, -17, -31
DTYPES = ["fp32", "fp16"]


@contextlib.contextmanager
def _route(value):
    """"sparse_inverted_build" set to `value`, the previous value restored afterwards"""
    from zvec_amd import _lib
    L = _lib.lib()
    before = C.c_int(0)
    assert L.zvec_hip_get_option(b"sparse_inverted_build", C.byref(before)) == 0
    assert L.zvec_hip_set_option(b"sparse_inverted_build", value) == 0
    try:
        yield
    finally:
        assert L.zvec_hip_set_option(b"sparse_inverted_build", before.value) == 0


def _B():
    import zvec_amd as zv
    return zv.HipFlatSparseStreamer().inverted_build_info()["block_elems"]


def _append(se, case, a=0, b=None):
    counts, idx, val = case
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    b = len(counts) if b is None else b
    assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]]) == 0


def _index(case, dtype, inverted=True):
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer(dtype=dtype)
    if inverted:
        se.set_inverted(True)
    if len(case[0]):
        _append(se, case)
    return se


def _export(se):
    terms, list_off, ppos, pval = se.inverted_export()
    return terms, list_off, ppos, M.raw(pval)


def _assert_same(got, want, what):
    for name, x, y in zip(("terms", "list_off", "ppos", "pval"), got, want):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            at = int(np.nonzero(x != y)[0][0])
            raise AssertionError("%s: %s differs first at %d: %r != %r" % (what, name, at, x[at], y[at]))


def _three_way(case, dtype, passes=None):
    """a device build, a host build on a second handle and the model agree bit for bit; returns the device build's handle"""
    want = M.twin_model(*case)
    with _route(1):
        dev = _index(case, dtype)
        got_dev = _export(dev)
        info = dev.inverted_build_info()
    assert info["route"] == 1 and info["passes"] == (M.passes_of(case[1]) if passes is None else passes) and info["ms"] > 0.0
    assert dev.inverted_info()["builds"] == 1 and dev.inverted_info()["terms"] == want[0].size
    with _route(0):
        host = _index(case, dtype)
        got_host = _export(host)
        hinfo = host.inverted_build_info()
    assert hinfo["route"] == 0 and hinfo["passes"] == 0 and hinfo["block_elems"] == info["block_elems"]
    _assert_same(got_host, want, "host build against the model")
    _assert_same(got_dev, want, "device build against the model")
    _assert_same(got_dev, got_host, "device build against host build")
    assert dev.inverted_info()["bytes"] == host.inverted_info()["bytes"]          # (the arrays have the host build's sizes)
    return dev


def _search(se, queries, k, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(k)
    if exclude is not None:
        ctx.set_exclude_bitset(exclude)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
    return ctx.keys.copy(), ctx.scores.copy(), ctx.counts.copy()


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


# ---- 1. block and wave edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", range(8))
def test_block_and_wave_edges(which, dtype):
    B = _B()
    E = M.edge_sizes(B)[which]
    case = M.edge_case(E, dtype)
    assert case[1].size == E
    _three_way(case, dtype)


# ---- 2. stability across lanes, waves and work-groups ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_list_keeps_position_order(dtype):
    B = _B()
    case = M.single_list_case(B, dtype)
    dev = _three_way(case, dtype)
    terms, list_off, ppos, pval = _export(dev)
    n = 2 * B + 5
    assert terms.tolist() == [77] and list_off.tolist() == [0, n]
    assert np.array_equal(ppos, np.arange(n, dtype=np.uint32))
    assert pval.tobytes() == M.raw(case[2]).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_alternating_indices_share_the_low_byte(dtype):
    B = _B()
    case = M.alternating_case(B, dtype)
    dev = _three_way(case, dtype, passes=2)
    terms, list_off, ppos, _ = _export(dev)
    n = 2 * B + 5
    assert terms.tolist() == [0x0105, 0x0305]
    assert np.array_equal(ppos[:int(list_off[1])], np.arange(1, n, 2, dtype=np.uint32))
    assert np.array_equal(ppos[int(list_off[1]):], np.arange(0, n, 2, dtype=np.uint32))


# ---- 3. pass count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pool,want", M.PASS_CASES)
def test_pass_count_comes_from_the_indices(name, pool, want):
    for dtype in DTYPES:
        case, w = M.pass_case(name, dtype)
        assert w == want and int(case[1].max()) == max(pool) and int(case[1].min()) == min(pool)
        _three_way(case, dtype, passes=want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_low_digit_is_still_a_pass(dtype):
    case = M.zero_low_digit_case(dtype)
    assert not np.any(case[1] & 255) and int(case[1].max()) < 65536
    _three_way(case, dtype, passes=2)


# ---- 4. rows and rebuilds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_and_a_row_across_a_block_boundary(dtype):
    B = _B()
    case = M.ragged_case(B, dtype)
    counts = case[0]
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    long_row = int(np.nonzero(counts == 300)[0][0])
    assert B < 300 or off[long_row] < B < off[long_row + 1]
    assert counts[-1] == 0 and np.any(counts[:long_row] == 0)
    _three_way(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [5, 0])
def test_no_elements(rows, dtype):
    case = M.empty_rows_case(dtype) if rows else M.no_rows_case(dtype)
    assert len(case[0]) == rows
    dev = _three_way(case, dtype, passes=0)
    terms, list_off, ppos, pval = _export(dev)
    assert terms.size == 0 and list_off.tolist() == [0] and ppos.size == 0 and pval.size == 0
    assert dev.inverted_info()["terms"] == 0
    # a search answers as it does on the host route and without the twin
    queries = (np.array([2, 0], np.uint32), np.array([1, 5], np.uint32), np.array([1, 2], M.np_dtype(dtype)))
    got = _search(dev, queries, 3)
    with _route(0):
        host = _index(case, dtype)
        want = _search(host, queries, 3)
    plain = _search(_index(case, dtype, inverted=False), queries, 3)
    assert got[2].tolist() == want[2].tolist() == plain[2].tolist() == [min(3, rows)] * 2
    for q in range(2):
        c = int(got[2][q])
        assert got[0][q, :c].tobytes() == want[0][q, :c].tobytes() and got[1][q, :c].tobytes() == want[1][q, :c].tobytes()
        assert got[1][q, :c].tobytes() == plain[1][q, :c].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_append_after_a_build_rebuilds_once_on_the_route_of_the_option(dtype):
    import zvec_amd as zv
    B = _B()
    case = M.edge_case(2 * B + 300, dtype, seed=7)
    n = len(case[0])
    n0, n1 = n // 2, n // 2 + n // 4
    cut = lambda m: (case[0][:m], case[1][:int(case[0][:m].sum())], case[2][:int(case[0][:m].sum())])      # noqa: E731
    queries = (np.array([2], np.uint32), case[1][:2].copy(), np.ones(2, M.np_dtype(dtype)))
    with _route(1):
        se = zv.HipFlatSparseStreamer(dtype=dtype)
        se.set_inverted(True)
        _append(se, case, 0, n0)
        _search(se, queries, 5)
        assert se.inverted_info()["builds"] == 1 and se.inverted_build_info()["route"] == 1
        _assert_same(_export(se), M.twin_model(*cut(n0)), "first build")
        _append(se, case, n0, n1)
        assert se.inverted_info()["builds"] == 1
        _search(se, queries, 5)
        assert se.inverted_info()["builds"] == 2 and se.inverted_build_info()["route"] == 1
        _assert_same(_export(se), M.twin_model(*cut(n1)), "rebuild on the device")
        assert se.inverted_info()["builds"] == 2                        # (the export of current lists builds nothing)
        # the option is read when a build starts: the next rebuild is the host's, to the same bytes
        with _route(0):
            _append(se, case, n1, n)
            _search(se, queries, 5)
            info = se.inverted_build_info()
            assert se.inverted_info()["builds"] == 3 and info["route"] == 0 and info["passes"] == 0
            on_host = _export(se)
        _assert_same(on_host, M.twin_model(*case), "rebuild on the host")
        whole = _index(case, dtype)
        _assert_same(_export(whole), on_host, "device build of all rows against the host rebuild")
        assert whole.inverted_build_info()["route"] == 1


# ---- 5. search answers across routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_answers_are_the_same_on_both_routes(dtype):
    n, vocab, nq, k = 3000, 2000, 16, 10
    rows = M.zipf_case(n, vocab, dtype)
    queries = M.zipf_case(nq, vocab, dtype, seed=27)
    mask = np.random.default_rng(28).random(n) < 0.3
    words = _words_of(mask)
    with _route(1):
        dev = _index(rows, dtype)
        got_dev = _search(dev, queries, k, exclude=words)
        assert dev.inverted_build_info()["route"] == 1
    with _route(0):
        host = _index(rows, dtype)
        got_host = _search(host, queries, k, exclude=words)
        assert host.inverted_build_info()["route"] == 0
    for a, b in zip(got_dev, got_host):
        assert a.tobytes() == b.tobytes()
    # the uninverted handle: the same score bits (the data are exact), the same keys up to the tie at the k-th place
    plain = _search(_index(rows, dtype, inverted=False), queries, k, exclude=words)
    assert got_dev[2].tobytes() == plain[2].tobytes() and got_dev[1].tobytes() == plain[1].tobytes()
    assert int(got_dev[2].min()) == k
    for q in range(nq):
        kth = plain[1][q, k - 1]
        assert {int(x) for x, s in zip(got_dev[0][q], got_dev[1][q]) if s < kth} == {int(x) for x, s in zip(plain[0][q], plain[1][q]) if s < kth}
        assert not mask[got_dev[0][q].astype(np.int64)].any()


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_device_builds_give_the_same_bytes(dtype):
    B = _B()
    case = M.edge_case(3 * B + 17, dtype, seed=3)
    with _route(1):
        se = _index(case, dtype)
        first = _export(se)
        se.set_inverted(False)                                          # drops the lists: the next export builds them again
        assert se.inverted_build_info()["route"] == -1
        se.set_inverted(True)
        second = _export(se)
        assert se.inverted_info()["builds"] == 2 and se.inverted_build_info()["route"] == 1
        third = _export(_index(case, dtype))
    _assert_same(second, first, "second build of the same handle")
    _assert_same(third, first, "build of a second handle")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    L = _lib.lib()
    before = C.c_int(-5)
    assert L.zvec_hip_get_option(b"sparse_inverted_build", C.byref(before)) == 0 and before.value in (0, 1)
    assert L.zvec_hip_set_option(b"sparse_inverted_build", 2) == INVALID and L.zvec_hip_set_option(b"sparse_inverted_build", -1) == INVALID
    now = C.c_int(-5)
    assert L.zvec_hip_get_option(b"sparse_inverted_build", C.byref(now)) == 0 and now.value == before.value
    # nothing built yet: the constant is there, the rest says so
    se = zv.HipFlatSparseStreamer()
    info = se.inverted_build_info()
    assert info["block_elems"] > 0 and info["route"] == -1 and info["passes"] == 0
    # no twin asked for
    nt, ne = C.c_uint64(7), C.c_uint64(7)
    assert L.zvec_hip_sparse_inverted_export(se._h, None, 0, None, None, None, 0, C.byref(nt), C.byref(ne)) == UNSUPPORTED
    # capacities
    case = M.edge_case(100, "fp32")
    with _route(1):
        on = _index(case, "fp32")
        assert L.zvec_hip_sparse_inverted_export(on._h, None, 0, None, None, None, 0, C.byref(nt), C.byref(ne)) == 0
    assert ne.value == 100 and nt.value == np.unique(case[1]).size
    terms, list_off = np.zeros(nt.value, np.uint32), np.zeros(nt.value + 1, np.uint64)
    ppos, pval = np.zeros(100, np.uint32), np.zeros(100, np.float32)
    args = lambda tc, ec: (on._h, _np_ptr(terms), tc, _np_ptr(list_off), _np_ptr(ppos), _np_ptr(pval), ec, None, None)      # noqa: E731
    assert L.zvec_hip_sparse_inverted_export(*args(nt.value - 1, 100)) == OUT_OF_RANGE
    assert L.zvec_hip_sparse_inverted_export(*args(nt.value, 99)) == OUT_OF_RANGE
    assert not terms.any() and not ppos.any()                           # (a refused call copies nothing)
    assert L.zvec_hip_sparse_inverted_export(*args(nt.value, 100)) == 0
    _assert_same((terms, list_off, ppos, M.raw(pval)), M.twin_model(*case), "export into the caller's arrays")
    # only the postings, with no room for terms: the capacity of an array that is not asked for does not matter
    assert L.zvec_hip_sparse_inverted_export(on._h, None, 0, None, _np_ptr(ppos), None, 100, None, None) == 0
    # NULL handles
    assert L.zvec_hip_sparse_inverted_export(None, None, 0, None, None, None, 0, C.byref(nt), C.byref(ne)) == INVALID
    assert L.zvec_hip_sparse_inverted_build_info(None, None, None, None, None) == INVALID
    assert L.zvec_hip_sparse_inverted_build_info(on._h, None, None, None, None) == 0

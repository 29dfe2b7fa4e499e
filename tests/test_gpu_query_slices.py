"""Every query-sliced search path past its first slice (q0 != 0) against plain references — run with -m gpu.

Six host loops cut a batch of queries into slices of at most 1 GiB of scores (or 32768 queries) and address the slice's queries,
norms, shared bounds, score rows and output rows at an offset q0.  tests/slices_ref.py holds one fixture per loop (2^20 + 37 rows
and 300 queries: slices of 255 and 45; or 200 rows and 32770 queries: slices of 32768 and 2), tests/test_slices_reference_cpu.py
holds the fixtures to "at least two slices" and to "the answers on the two sides of a boundary differ".  Here every test runs
ONE search per variant and checks query 0, the last query and three queries on each side of every boundary against a reference
computed for those queries alone.  All data are small integers: every score is exact and the lists are held exactly, the rows at
the k-th score and the order of equal scores being the only freedom.  Every assertion names the query and its slice.

  loop  test                                   index                                   what is offset by q0 and checked here
  1     test_flat_large_k                      HipFlatSearcher fp32, L2 and IP         qpad, qnorm (L2, a planted pair of norms), out rows,
                                                                                       out.idx for refine_l2 (gtau + q0 is not: the dump reads no bound)
  2     test_hamming_large_k                   HipFlatSearcher binary32                queries, out rows
  3     test_sparse_scan_large_k               HipFlatSparseStreamer fp32 and fp16     plan blocks, dump rows, out rows
  4     test_sparse_inverted                   the fp32 one with its term-major twin   a.q0, a.nq, out rows
  5     test_sparse_grouped_score_matrix       the fp32 one                            qsub0 / plan blocks, group_select's outputs
  5     test_sparse_grouped_32768[scan]        200 rows                                the same, second slice by the wave-per-row dump
  6     test_sparse_grouped_32768[by_ids]      200 rows                                part_s / part_i rows, group_select's outputs"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slices_ref as S  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
ROUTE_DENSE, ROUTE_COMPACT, ROUTE_EXCL = 1 << 0, 1 << 8, 1 << 9          # zvec_hip_ctx_last_route (api_flat_scan.inc.h)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _each_checked(fx, check):
    """check(j, query) for every checked query; a failure names the query and its slice"""
    for j, qi in enumerate(S.checked_queries(fx)):
        try:
            check(j, qi)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (S.where(fx, qi), e)) from e


def _flat_lists(se, q, k, exclude_words=None):
    ctx = se.create_context()
    ctx.set_topk(k)
    if exclude_words is not None:
        ctx.set_exclude_bitset(exclude_words)
    assert se.search_impl(q, len(q), ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts, ctx.last_route()


# ---- loop 1: flat, large k -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", S.FIXTURES["flat_large_k"]["metrics"])
def test_flat_large_k(metric):
    """k = 600 is beyond the fused lists: the dense-score path, 300 queries over 2^20 + 37 rows in slices of 255 and 45.
    InnerProduct has no refinement behind it: a wrong query row shows in the scores as they leave the scan.  SquaredEuclidean
    adds refine_l2, which re-scores the positions of ALL slices after the loop (out.idx at q0 * k), and qnorm + q0: query 255
    carries the largest norm and query 0 a tiny one (slices_ref.dense_data), so that scored with query 0's norm most rows of
    query 255 clamp to 0 and its list is not the 600 nearest (held on the CPU, test_a_norm_that_is_not_offset_changes_the_l2_answer).
    gtau + q0 is not checked: the scan's dump mode reads no shared bound.  InnerProduct is run a second time with 45 % of the
    rows excluded: the bitset is shared by the slices and must not be offset."""
    import zvec_amd as zv
    fx = S.FIXTURES["flat_large_k"]
    n, k = fx["n"], fx["k"]
    base, q = S.dense_data()
    key_of = S.sparse_key_of(n)
    se = zv.HipFlatSearcher(fx["dim"], metric, dtype=fx["dtype"])
    assert se.load(base, key_of) == 0 and se.count() == n
    ref = S.dense_reference(metric)
    variants = [("plain", None)] + ([("exclude", S.exclude_mask(n))] if metric == "InnerProduct" else [])
    for tag, mask in variants:
        keys, scores, counts, route = _flat_lists(se, q, k, None if mask is None else S.words_of(mask))
        assert route & ROUTE_DENSE, "%s %s: route %#x is not the dense-score path" % (metric, tag, route)
        assert not route & ROUTE_COMPACT and bool(route & ROUTE_EXCL) == (mask is not None), "%s %s: route %#x" % (metric, tag, route)
        adm = None if mask is None else ~mask
        pos, want_s, want_c = S.top_lists(ref, k, adm)
        want_k = key_of[pos.astype(np.int64)]

        def check(j, qi):
            what = "%s %s" % (metric, tag)
            U.tie_tolerant_compare(keys[qi:qi + 1], scores[qi:qi + 1], counts[qi:qi + 1], want_k[j:j + 1], want_s[j:j + 1], want_c[j:j + 1], what=what)
            S.check_exact_list(keys[qi], scores[qi], counts[qi], ref[j], k, key_of, adm, what=what)
        _each_checked(fx, check)
    del se
    S.drop("ref_dense")


# ---- loop 2: Hamming, k = 129 --------------------------------------------------------------------------------------------------------
def test_hamming_large_k():
    """k = 129 is beyond HAM_FUSED_MAX_K: the dense [query][position] matrix of distances, in slices of 255 and 45 queries; a
    32-query block of the uncut batch would straddle query 255"""
    import zvec_amd as zv
    fx = S.FIXTURES["hamming"]
    n, k = fx["n"], fx["k"]
    base, q = S.hamming_data()
    key_of = S.sparse_key_of(n)
    se = zv.HipFlatSearcher(fx["dim"], "Hamming", dtype=fx["dtype"])
    assert se.add_batch(base, key_of) == 0 and se.count() == n
    keys, scores, counts, _ = _flat_lists(se, q, k)
    ref = S.hamming_scores().astype(np.float64)
    _each_checked(fx, lambda j, qi: S.check_exact_list(keys[qi], scores[qi], counts[qi], ref[j], k, key_of, what="hamming"))
    del se
    S.drop("ref_hamming")


# ---- loops 3 - 5: sparse rows, one index per value type for the module ----------------------------------------------------------------
_SPARSE = {}


def _sparse_index(n, dtype="fp32"):
    """(streamer, context), built once per module; keys = position * 3 + 7, appended in two pieces"""
    import zvec_amd as zv
    if (n, dtype) not in _SPARSE:
        counts, idx, val = S.sparse_rows(n)
        off = S.R.offsets(counts)
        se = zv.HipFlatSparseStreamer(dtype=dtype)
        key_of = S.sparse_key_of(n)
        for a, b in ((0, n // 2), (n // 2, n)):
            assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], key_of[a:b]) == 0
        assert se.count() == n
        _SPARSE[(n, dtype)] = (se, se.create_context())
    return _SPARSE[(n, dtype)]


@pytest.fixture(scope="module", autouse=True)
def _drop_indexes():
    yield
    _SPARSE.clear()
    S.drop("")


def _sparse_lists(se, queries, k):
    ctx = se.create_context()
    ctx.set_topk(k)
    assert se.search_impl(queries[0], queries[1], queries[2], len(queries[0]), ctx) == 0
    return ctx.keys, ctx.scores, ctx.counts


def _check_sparse(name, got, what):
    fx = S.FIXTURES[name]
    keys, scores, counts = got
    ref = S.sparse_case(name)[2]
    key_of = S.sparse_key_of(fx["n"])
    _each_checked(fx, lambda j, qi: S.check_exact_list(keys[qi], scores[qi], counts[qi], ref[j], fx["k"], key_of, what=what))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_sparse_scan_large_k(dtype):
    """k = 129 is beyond SPARSE_FUSED_MAX_K: sparse_search_locked dumps [query][n] scores in slices of 255 and 45 queries.  255 is
    no multiple of the 64-query plan block: sparse_make_plan has to cut a block at query 255, sparse_dump_scores has to find
    the blocks of a slice, and the kernel writes row (q - qsub0) of the dump.  fp16 values share all of it (sparse_dispatch picks
    the kernel's value type inside the same loop) with a query image of another width; the integers are exact in both."""
    fx = S.FIXTURES["sparse_scan"]
    se, _ = _sparse_index(fx["n"], dtype)
    assert not se.inverted_info()["enabled"]
    got = _sparse_lists(se, S.sparse_queries(fx["count"]), fx["k"])
    _check_sparse("sparse_scan", got, "sparse scan %s" % dtype)
    if dtype == "fp16":
        del _SPARSE[(fx["n"], dtype)]


def test_sparse_inverted():
    """the same rows through the term-major twin, k = 10: every k takes the [query][whole 4096-row tiles] matrix, in slices of
    255 and 45 queries.  Held to the reference, and to the row scan's answer at the same k (scores equal; keys equal below the
    k-th score, as tests/test_gpu_sparse_inverted.py compares the two)."""
    fx = S.FIXTURES["sparse_inverted"]
    k = fx["k"]
    se, _ = _sparse_index(fx["n"])
    queries = S.sparse_queries(fx["count"])
    scan = _sparse_lists(se, queries, k)
    se.set_inverted(True)
    try:
        twin = _sparse_lists(se, queries, k)
        assert se.inverted_info()["enabled"] and se.inverted_info()["builds"] >= 1
    finally:
        se.set_inverted(False)
    _check_sparse("sparse_inverted", twin, "sparse twin")

    def same(j, qi):
        assert twin[2][qi] == scan[2][qi] == k
        assert np.array_equal(twin[1][qi], scan[1][qi]), "twin scores %r, row scan %r" % (twin[1][qi], scan[1][qi])
        kth = scan[1][qi][k - 1]
        a = {int(x) for x, s in zip(twin[0][qi], twin[1][qi]) if s < kth}
        b = {int(x) for x, s in zip(scan[0][qi], scan[1][qi]) if s < kth}
        assert a == b, "twin keys %r, row scan %r below the k-th score" % (sorted(a), sorted(b))
    _each_checked(fx, same)


@contextlib.contextmanager
def _group_rows(value):
    """"sparse_group_rows" set to `value` (None: left alone), the previous value restored afterwards"""
    from zvec_amd import _lib
    L = _lib.lib()
    before = C.c_int(-1)
    assert L.zvec_hip_get_option(b"sparse_group_rows", C.byref(before)) == 0
    if value is not None:
        assert L.zvec_hip_set_option(b"sparse_group_rows", value) == 0
    try:
        yield before.value
    finally:
        assert L.zvec_hip_set_option(b"sparse_group_rows", before.value) == 0


def _grouped(name, lists=None):
    """the C ABI call of a grouped fixture: (groups, ngroups, keys, scores, counts) of ALL its queries"""
    from zvec_amd import _lib
    L = _lib.lib()
    fx = S.FIXTURES[name]
    se, ctx = _sparse_index(fx["n"])
    c, i, v = [np.ascontiguousarray(a) for a in S.sparse_queries(fx["count"])]
    count, gnum, gk = fx["count"], fx["gnum"], fx["gk"]
    gof = np.ascontiguousarray(S.group_of(name), np.uint32)
    out = (np.full((count, gnum), 0xdeadbeef, np.uint32), np.full(count, 0xdeadbeef, np.uint32), np.zeros((count, gnum, gk), np.uint64),
           np.zeros((count, gnum, gk), np.float32), np.full((count, gnum), 0xdeadbeef, np.uint32))
    if lists is None:
        rc = L.zvec_hip_sparse_search_grouped(se._h, ctx._h, _ptr(c), _ptr(i), _ptr(v), count, _ptr(gof), fx["ngroups"], gnum, gk,
                                              C.c_float(FLT_MAX), None, *[_ptr(a) for a in out])
    else:
        ids = np.concatenate(list(lists) + [np.zeros(1, np.uint32)]).astype(np.uint32)
        offs = np.zeros(count + 1, np.uint32)
        offs[1:] = np.cumsum([len(a) for a in lists])
        rc = L.zvec_hip_sparse_search_grouped_by_ids(se._h, ctx._h, _ptr(c), _ptr(i), _ptr(v), count, _ptr(ids), _ptr(offs), _ptr(gof),
                                                     fx["ngroups"], gnum, gk, C.c_float(FLT_MAX), None, *[_ptr(a) for a in out])
    assert rc == 0
    return out


def _check_grouped(name, got, what):
    fx = S.FIXTURES[name]
    want = S.group_want(name)
    _each_checked(fx, lambda j, qi: S.G.check_exact(tuple(a[j:j + 1] for a in want), tuple(a[qi:qi + 1] for a in got), what))


@pytest.mark.parametrize("wave_rows", [None, 64], ids=["default", "rows64"])
def test_sparse_grouped_score_matrix(wave_rows):
    """zvec_hip_sparse_search_grouped over 2^20 + 37 rows: slices of 255 and 45 queries, every list held bit for bit.  At the
    default "sparse_group_rows" (at most 45 is asserted) both slices are dumped lane = query through the cut plan; at 64 the
    second slice is dumped a wave per row, sparse_rows_dump_kernel with qsub0 = 255."""
    name = "sparse_group_gib"
    with _group_rows(wave_rows) as default:
        assert default < S.FIXTURES[name]["count"] - S.slice_width(S.FIXTURES[name]) <= 64
        got = _grouped(name)
    _check_grouped(name, got, "sparse grouped, sparse_group_rows %r" % wave_rows)


@pytest.mark.parametrize("by_ids", [False, True], ids=["scan", "by_ids"])
def test_sparse_grouped_32768(by_ids):
    """32770 queries over 200 rows: both grouped entry points slice at 32768, which leaves a second slice of two queries (the full
    scan dumps it a wave per row, qsub0 = 32768; by-ids hands group_select rows 32768.. of the candidate matrix)"""
    name = "sparse_group_ids_32768" if by_ids else "sparse_group_32768"
    with _group_rows(None) as rows:
        assert rows >= 2, "sparse_group_rows %d: the second slice would not be dumped a wave per row" % rows
    got = _grouped(name, S.id_lists(name) if by_ids else None)
    _check_grouped(name, got, "sparse grouped 32768 by_ids=%r" % by_ids)

"""HNSW on IEEE binary16 rows on the GPU (zvec_hip_hnsw_create_typed(ZVEC_HIP_DT_FP16)), on the fixtures of tests/hnsw_f16_ref.py.
The contract (DESIGN §3c "fp16 rows"): a half is widened exactly and the arithmetic from there on is the fp32 kernel's own, so an fp16
handle answers bit for bit as W, the fp32 handle given the widened rows and queries.  On exact data (integers, exact in binary16, every
distance an exact fp32 integer) the fp64 models of hnsw_ref / hnsw_build_ref / hnsw_add_ref apply to the fp16 handle as they stand; on
real data (Gaussian halves, with subnormals, -0.0 and the largest half planted) the fp16 handle is compared with W: lists, counts,
statistics, exported graphs and counters.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_add_ref as A  # noqa: E402
import hnsw_build_ref as B  # noqa: E402
import hnsw_f16_ref as F  # noqa: E402
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, MISMATCH, INVALID, NO_INDEX_LOADED = -12, -24, -31, -204
NAMES = {"l2": "SquaredEuclidean", "ip": "InnerProduct"}
NOKEY = 0xffffffffffffffff
OPTIONS = {"hnsw_build_round_div": 16, "hnsw_build_round_max": 4096, "hnsw_ws_bytes": 1 << 30}
COUNTERS = ("rounds", "slices", "top", "entry_point", "dists", "requests", "prunes")        # (not the millisecond fields)
ADD_COUNTERS = COUNTERS + ("first", "count", "rounds_one", "grew_rows", "grew_upper", "restrided", "cap_rows", "cap_upper")
_keys = A._keys


class _options:
    """run-time options for the length of a with block; the defaults come back afterwards"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from zvec_amd import _lib
        for k, v in self.kw.items():
            _lib.check(_lib.lib().zvec_hip_set_option(k.encode(), int(v)), "set_option")

    def __exit__(self, *exc):
        from zvec_amd import _lib
        for k in self.kw:
            _lib.check(_lib.lib().zvec_hip_set_option(k.encode(), OPTIONS[k]), "set_option")


def _searcher(dim, metric="l2", dtype="fp16"):
    import zvec_amd as zv
    return zv.HipHnswSearcher(dim, NAMES[metric], dtype=dtype)


def _rows_for(se, rows16):
    """the twin's rows as this handle takes them: the halves, or their widened values for W"""
    return rows16 if se.np_dtype is np.float16 else F.widen(rows16)


def _loaded(g, rows16, metric="l2", dtype="fp16"):
    se = _searcher(rows16.shape[1], metric, dtype)
    up = g.max_level > 0
    assert se.load(_rows_for(se, rows16), g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of if up else None, g.nbr_up if up else None,
                   g.cnt_up if up else None) == 0
    return se


def _search(se, q16, topk, ef, max_scan=0, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(topk)
    if threshold is not None:
        ctx.set_threshold(threshold)
    ctx.set_exclude_bitset(None if exclude is None else H.words_of(exclude))
    assert se.search(_rows_for(se, q16), q16.shape[0], ctx, ef, max_scan) == 0
    scanned, hops, slices = se.last_stats(ctx, q16.shape[0])
    return ctx.keys, ctx.scores, ctx.counts, scanned, hops, slices


def _same_bits(a, b, what=""):
    """two search results: keys, scores (by their bits), counts, distances computed, nodes expanded, slices"""
    for x, y, name in zip(a, b, ("keys", "scores", "counts", "scanned", "hops", "slices")):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), "%s: %s" % (what, name)


def _against_model(se, g, q16, topk, ef, metric="l2", max_scan=0, what=""):
    keys, scores, counts, scanned, hops, _ = _search(se, q16, topk, ef, max_scan)
    for i in range(q16.shape[0]):
        r = H.search_model(g, F.widen(q16[i]), topk, ef, max_scan, metric=metric)
        w = "%s query %d" % (what, i)
        assert counts[i] == r.keys.size, w
        assert np.array_equal(keys[i, :counts[i]], r.keys) and np.array_equal(scores[i, :counts[i]], r.scores), w
        assert (keys[i, counts[i]:] == NOKEY).all() and np.isinf(scores[i, counts[i]:]).all(), w
        assert (scanned[i], hops[i]) == (r.scanned, r.hops), w


def _export_equal(a, b, what=""):
    ia, ib = a.info(), b.info()
    assert ia == ib, what
    for x, y in zip(a.export(), b.export()):
        assert (x is None) == (y is None), what
        if x is not None:
            assert x.dtype == y.dtype and np.array_equal(x, y), what


def _same_graph(se, g, rows16, what=""):
    """the handle holds the model's graph, array for array, and the halves that went in"""
    i = se.info()
    n = g.rows.shape[0]
    assert (i["n"], i["m0"], i["max_level"], i["entry_point"]) == (n, g.m0, g.max_level, g.entry_point), what
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    assert np.array_equal(keys, g.keys) and np.array_equal(cnt0, g.cnt0) and np.array_equal(nbr0, g.nbr0), what
    if g.max_level > 0:
        assert (i["m"], i["n_upper"]) == (g.m, g.n_upper), what
        assert np.array_equal(upper_of, g.upper_of) and np.array_equal(cnt_up, g.cnt_up) and np.array_equal(nbr_up, g.nbr_up), what
    else:
        assert upper_of is None, what
    got = se.get_vectors_by_ids(np.arange(n))
    assert got.dtype == np.float16 and got.tobytes() == rows16[:n].tobytes(), what


def _params(p):
    return dict(m=p.m, m0=p.m0, ef_construction=p.ef_construction, prune_cnt=p.prune_cnt, min_neighbors=p.min_neighbors,
                scaling_factor=p.scaling_factor)


def _pick(info, names):
    return tuple(int(info[k]) for k in names)


# ---- against the fp64 models, exactly, on exact data -----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", F.EXACT_DIMS)
def test_exact_search_equals_the_model(dim, metric):
    t = F.exact_twin(dim)
    se = _loaded(t.graph, t.rows16, metric)
    for ef in (5, 64, 512):
        _against_model(se, t.graph, t.queries16, 5, ef, metric, what="dim=%d %s ef=%d" % (dim, metric, ef))


@pytest.mark.parametrize("name", list(F.usable_hand_made()))
def test_hand_made_graphs(name):
    g = F.usable_hand_made()[name]()
    se = _loaded(g, g.rows.astype(np.float16))
    for ef, topk in ((1, 1), (3, 3), (8, 64), (64, 8)):
        _against_model(se, g, F.HAND_QUERIES, topk, ef, what="%s ef=%d topk=%d" % (name, ef, topk))
    _against_model(se, g, F.HAND_QUERIES, 5, 5, max_scan=3, what=name + " max_scan=3")


@pytest.mark.parametrize("round_div", [16, 0])
@pytest.mark.parametrize("dim", [5, 64])
def test_exact_build_equals_the_model(dim, round_div):
    rows16, p, lv = F.build_rows(300, dim)
    g, c = B.build_model(F.widen(rows16), p, lv, round_div, 4096, "l2", keys=_keys(300))
    se = _searcher(dim)
    with _options(hnsw_build_round_div=round_div):
        assert se.build(rows16, keys=_keys(300), levels=lv, **_params(p)) == 0
    _same_graph(se, g, rows16, "build dim=%d round_div=%d" % (dim, round_div))
    b = se.build_info()
    print("gpu", _pick(b, ("rounds", "dists", "requests", "prunes")), "model", tuple(c))
    assert _pick(b, ("rounds", "dists", "requests", "prunes")) == tuple(c)
    assert (b["top"], b["entry_point"]) == (g.max_level, g.entry_point)


@pytest.mark.parametrize("start", ["empty", "loaded"])
def test_exact_add_equals_the_model(start):
    """200 rows, then calls of 1, 9 and 90: from an empty handle (the first call is an add that builds) and from a loaded graph"""
    rows16, p, lv = F.build_rows(300, 24)
    calls = A.add_model(F.widen(rows16), p, lv, (200, 1, 9, 90), 16, 4096, "l2", keys=_keys(300))
    se = _searcher(24)
    g0 = calls[0].graph
    if start == "empty":
        assert se.add(rows16[:200], keys=_keys(300)[:200], levels=lv[:200], **_params(p)) == 0
        assert _pick(se.add_info(), ("rounds", "dists", "requests", "prunes")) == tuple(calls[0].counters)
    else:
        assert se.load(rows16[:200], g0.nbr0, g0.cnt0, g0.entry_point, keys=g0.keys, upper_of=g0.upper_of, nbr_up=g0.nbr_up,
                       cnt_up=g0.cnt_up) == 0
    _same_graph(se, g0, rows16, start)
    for k in calls[1:]:
        a, e = k.first, k.first + k.count
        assert se.add(rows16[a:e], keys=_keys(300)[a:e], levels=lv[a:e], **_params(p)) == 0
        i = se.add_info()
        assert _pick(i, ("rounds", "dists", "requests", "prunes")) == tuple(k.counters), (start, a)
        assert (i["first"], i["count"], i["top"], i["entry_point"]) == (a, k.count, k.graph.max_level, k.graph.entry_point)
        _same_graph(se, k.graph, rows16, "%s, call at %d" % (start, a))


# ---- against the widened fp32 twin W, bit for bit, on real data -------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", F.REAL_DIMS)
def test_real_search_equals_the_twin(dim, metric):
    t = F.real_twin(dim)
    h, w = _loaded(t.graph, t.rows16, metric), _loaded(t.graph, t.rows16, metric, "fp32")
    q = t.queries16
    _same_bits(_search(h, q, 10, 64), _search(w, q, 10, 64), "plain")
    ex = np.arange(F.REAL_N) % 3 == 0
    _same_bits(_search(h, q, 10, 32, exclude=ex), _search(w, q, 10, 32, exclude=ex), "exclude bits")
    full = _search(w, q, 10, 64)
    thr = float(np.sort(full[1][:, 4])[q.shape[0] // 2])           # the fifth score of the median query: cuts some lists, not all
    a, b = _search(h, q, 10, 64, threshold=thr), _search(w, q, 10, 64, threshold=thr)
    assert 0 < int(b[2].sum()) < 10 * q.shape[0]
    _same_bits(a, b, "threshold")
    a, b = _search(h, q, 10, 64, max_scan=50), _search(w, q, 10, 64, max_scan=50)
    assert (b[3] >= 50).all() and (b[3] < full[3]).any()
    _same_bits(a, b, "max_scan 50")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_candidates_spill_into_the_workspace(metric):
    """n = 1500 with 1400 rows excluded: more than 1024 candidates alive (tests/test_hnsw_f16_reference_cpu.py shows it)"""
    t = F.spill_twin()
    h, w = _loaded(t.graph, t.rows16, metric), _loaded(t.graph, t.rows16, metric, "fp32")
    ex = F.spill_exclude()
    a, b = _search(h, t.queries16, 10, 512, exclude=ex), _search(w, t.queries16, 10, 512, exclude=ex)
    assert (b[3] >= F.SPILL_N).all()                                # (every row was computed: the walk never met a full R)
    _same_bits(a, b, "spill")


def test_query_slices():
    t = F.real_twin(68)
    h, w = _loaded(t.graph, t.rows16), _loaded(t.graph, t.rows16, dtype="fp32")
    q = t.queries16
    whole = _search(h, q, 10, 32)
    assert whole[5] == 1
    per_query = 4 * ((F.REAL_N + 31) // 32) + 8 * F.REAL_N           # visited words + the candidate region (include/zvec_hip.h)
    with _options(hnsw_ws_bytes=7 * per_query):
        a, b = _search(h, q, 10, 32), _search(w, q, 10, 32)
    assert a[5] == 4                                                # 24 queries, 7 a slice
    _same_bits(a, b, "4 slices")
    _same_bits(a[:5], whole[:5], "slices are invisible")


def test_search_dev_takes_halves_in_device_memory():
    import torch
    t = F.real_twin(772)
    h, w = _loaded(t.graph, t.rows16, "ip"), _loaded(t.graph, t.rows16, "ip", "fp32")
    q = t.queries16
    nq = q.shape[0]
    ex = np.arange(F.REAL_N) % 4 == 1
    want = _search(w, q, 10, 48, exclude=ex)
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    assert dq.dtype == torch.float16
    dex = torch.from_numpy(H.words_of(ex).view(np.int64)).to(dev)
    dk = torch.zeros((nq, 10), dtype=torch.int64, device=dev)
    ds = torch.zeros((nq, 10), dtype=torch.float32, device=dev)
    dc = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = h.create_context()
    assert h.search_dev(dq.data_ptr(), nq, 10, 48, 0, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx, d_exclude=dex.data_ptr()) == 0
    scanned, hops, slices = h.last_stats(ctx, nq)
    got = (dk.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dc.cpu().numpy().view(np.uint32), scanned, hops, slices)
    _same_bits(got, want, "search_dev")


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim", F.REAL_DIMS)
def test_real_build_and_adds_equal_the_twin(dim, metric):
    """build at n = 600, then adds of 1, 64 and 300 rows without a reserve (the rows array grows); after every call the export and
    the counters equal W's, and at the end every stored row is the half that went in"""
    p = F.BUILD_PARAMS
    total = F.BUILD_N + sum(F.BUILD_ADDS)
    rows16 = F.real_rows(total, dim, 7)
    lv = F.real_levels(total)
    keys = _keys(total)
    h, w = _searcher(dim, metric), _searcher(dim, metric, "fp32")
    n = F.BUILD_N
    for se in (h, w):
        assert se.build(_rows_for(se, rows16[:n]), keys=keys[:n], levels=lv[:n], **_params(p)) == 0
    assert _pick(h.build_info(), COUNTERS) == _pick(w.build_info(), COUNTERS)
    assert h.build_info()["prunes"] > 0
    _export_equal(h, w, "build")
    grew = False
    for count in F.BUILD_ADDS:
        for se in (h, w):
            assert se.add(_rows_for(se, rows16[n:n + count]), keys=keys[n:n + count], levels=lv[n:n + count]) == 0
        n += count
        ia, ib = h.add_info(), w.add_info()
        assert _pick(ia, ADD_COUNTERS) == _pick(ib, ADD_COUNTERS), count
        grew = grew or bool(ia["grew_rows"])
        _export_equal(h, w, "add of %d" % count)
    assert grew and n == total
    got = h.get_vectors_by_ids(np.arange(total))
    assert got.dtype == np.float16 and got.tobytes() == rows16.tobytes()
    q = F.real_rows(F.REAL_Q, dim, 8)
    _same_bits(_search(h, q, 10, 64), _search(w, q, 10, 64), "search after the adds")


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_planted_subnormals_minus_zero_and_the_largest_half(metric):
    t = F.planted_twin()
    h, w = _loaded(t.graph, t.rows16, metric), _loaded(t.graph, t.rows16, metric, "fp32")
    a, b = _search(h, t.queries16, 10, 128), _search(w, t.queries16, 10, 128)
    _same_bits(a, b, "planted search")
    # the walk is not steered to the planted rows: score them on purpose, with everything else excluded
    only = np.ones(F.REAL_N, bool)
    only[[F.PLANT_ROW, F.PLANT_MAX_ROW]] = False
    a, b = _search(h, t.queries16, 2, 512, exclude=only), _search(w, t.queries16, 2, 512, exclude=only)
    assert (b[2] == 2).all()
    assert (b[1][F.PLANT_QUERY] != 0).all()                         # the query of subnormals alone: nothing was flushed to zero
    _same_bits(a, b, "planted rows alone")
    # and a build over the planted rows
    n = 400
    p = F.BUILD_PARAMS
    lv = F.real_levels(n)
    hb, wb = _searcher(F.PLANT_DIM, metric), _searcher(F.PLANT_DIM, metric, "fp32")
    for se in (hb, wb):
        assert se.build(_rows_for(se, t.rows16[:n]), levels=lv, **_params(p)) == 0
    assert _pick(hb.build_info(), COUNTERS) == _pick(wb.build_info(), COUNTERS)
    _export_equal(hb, wb, "planted build")


# ---- plumbing and refusals --------------------------------------------------------------------------------------------------------
def test_dtype_and_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    L = _lib.lib()
    d = C.c_int(-1)
    for name, want in (("fp16", _lib.DT_FP16), ("fp32", _lib.DT_FP32)):
        se = zv.HipHnswSearcher(16, dtype=name)
        assert L.zvec_hip_hnsw_dtype(se._h, C.byref(d)) == 0 and d.value == want
    assert L.zvec_hip_hnsw_dtype(None, C.byref(d)) == INVALID and L.zvec_hip_hnsw_dtype(se._h, None) == INVALID
    out = C.c_void_p(0x55)
    assert L.zvec_hip_hnsw_create_typed(16, _lib.DT_BINARY32, _lib.METRIC_L2, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    assert L.zvec_hip_hnsw_create_typed(16, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    for dt in (_lib.DT_FP16, _lib.DT_FP32):
        assert L.zvec_hip_hnsw_create_typed(16, dt, _lib.METRIC_COSINE, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    assert L.zvec_hip_hnsw_create_typed(4097, _lib.DT_FP16, _lib.METRIC_L2, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55
    assert L.zvec_hip_hnsw_create_typed(0, _lib.DT_FP16, _lib.METRIC_L2, 0, C.byref(out)) == INVALID and out.value == 0x55
    assert L.zvec_hip_hnsw_create_typed(16, _lib.DT_FP16, _lib.METRIC_L2, 0, None) == INVALID
    assert L.zvec_hip_hnsw_create(16, _lib.DT_FP16, _lib.METRIC_L2, 0, C.byref(out)) == UNSUPPORTED and out.value == 0x55      # as before
    with pytest.raises(_lib.ZvecHipError):
        zv.HipHnswSearcher(16, dtype="binary32")
    se = zv.HipHnswSearcher(8, dtype="fp16")
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search(np.zeros((2, 8), np.float16), 2, ctx, 8) == NO_INDEX_LOADED
    assert se.load(np.zeros((3, 9), np.float16), np.zeros((3, 2), np.uint32), np.zeros(3, np.uint32)) == MISMATCH
    assert se.search(np.zeros((2, 8), np.float16), 2, ctx, 513) == UNSUPPORTED


def test_create_typed_fp32_is_create():
    import zvec_amd as zv
    from zvec_amd import _lib
    t = F.real_twin(64)
    plain = _loaded(t.graph, t.rows16, dtype="fp32")
    typed = zv.HipHnswSearcher.__new__(zv.HipHnswSearcher)                 # a searcher over a handle from create_typed(DT_FP32)
    typed.dim, typed.metric, typed.device, typed.dtype, typed.np_dtype, typed._h = 64, _lib.METRIC_L2, 0, _lib.DT_FP32, np.float32, C.c_void_p()
    assert _lib.lib().zvec_hip_hnsw_create_typed(64, _lib.DT_FP32, _lib.METRIC_L2, 0, C.byref(typed._h)) == 0
    g = t.graph
    assert typed.load(F.widen(t.rows16), g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of, g.nbr_up, g.cnt_up) == 0
    d = C.c_int(-1)
    assert _lib.lib().zvec_hip_hnsw_dtype(typed._h, C.byref(d)) == 0 and d.value == _lib.DT_FP32
    _same_bits(_search(typed, t.queries16, 10, 64), _search(plain, t.queries16, 10, 64), "typed fp32")
    assert typed.get_vectors_by_ids(np.arange(5)).dtype == np.float32


def test_float32_arrays_are_rounded_to_halves():
    """an fp16 searcher given float32 arrays (not half values) equals the same searcher given astype(float16) arrays"""
    rng = np.random.default_rng(12)
    n, dim = 500, 20
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((9, dim)).astype(np.float32)
    assert not F.is_half(rows) and not F.is_half(q)
    lv = F.real_levels(n)
    a, b = _searcher(dim), _searcher(dim)
    p = _params(F.BUILD_PARAMS)
    assert a.build(rows[:300], levels=lv[:300], **p) == 0 and b.build(rows[:300].astype(np.float16), levels=lv[:300], **p) == 0
    assert a.add(rows[300:], levels=lv[300:]) == 0 and b.add(rows[300:].astype(np.float16), levels=lv[300:]) == 0
    _export_equal(a, b, "float32 in")
    assert a.get_vectors_by_ids(np.arange(n)).tobytes() == rows.astype(np.float16).tobytes()
    ca, cb = a.create_context(), b.create_context()
    for c in (ca, cb):
        c.set_topk(10)
    assert a.search(q, 9, ca, 64) == 0 and b.search(q.astype(np.float16), 9, cb, 64) == 0
    _same_bits((ca.keys, ca.scores, ca.counts), (cb.keys, cb.scores, cb.counts), "float32 queries")
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = a.export()
    i = a.info()
    c = _searcher(dim)
    assert c.load(rows, nbr0, cnt0, i["entry_point"], keys, upper_of, nbr_up, cnt_up) == 0                 # load rounds too
    assert c.get_vectors_by_ids(np.arange(n)).tobytes() == rows.astype(np.float16).tobytes()


def test_empty_handle():
    se = _searcher(8)
    assert se.load(np.zeros((0, 8), np.float16), np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32)) == 0
    assert se.info()["n"] == 0
    keys, scores, counts, scanned, hops, _ = _search(se, np.ones((3, 8), np.float16), 4, 16)
    assert (counts == 0).all() and (keys == NOKEY).all() and np.isinf(scores).all() and (scanned == 0).all() and (hops == 0).all()
    assert se.build(np.zeros((0, 8), np.float16), m=8) == 0 and se.info()["n"] == 0
    assert se.get_vectors_by_ids(np.zeros(0, np.uint64)).shape == (0, 8)


def test_load_then_add_takes_the_defaults_as_fp32_does():
    """no parameters after a load: the reference's defaults (ef_construction 500, prune_cnt m, ...) with the graph's widths, on both"""
    t = F.real_twin(64)
    g = t.graph
    more = F.real_rows(40, 64, 9)
    lv = np.zeros(40, np.uint32)
    lv[7] = 1
    h, w = _loaded(g, t.rows16), _loaded(g, t.rows16, dtype="fp32")
    for se in (h, w):
        assert se.add(_rows_for(se, more), levels=lv) == 0
    ia, ib = h.add_info(), w.add_info()
    assert _pick(ia, ADD_COUNTERS) == _pick(ib, ADD_COUNTERS) and ia["count"] == 40 and ia["first"] == F.REAL_N
    assert h.info()["n"] == F.REAL_N + 40 and (h.info()["m0"], h.info()["m"]) == (g.m0, g.m)
    _export_equal(h, w, "load then add")
    # the walks ran with more than the graph's widths would suggest: ef_construction 500 computes far more distances than 32 would
    assert ia["dists"] > 40 * 500


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_fp16")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "hnsw_fp16.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_fp16 ok" in out.stdout.decode()

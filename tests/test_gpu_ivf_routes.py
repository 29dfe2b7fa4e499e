"""Every route of ivf_search_core from GIVEN probe lists against fp64 (tests/ivf_routes_ref.py) — run with -m gpu.

zvec_hip_ivf_search_probes_dev takes the probe lists from the test: no coarse ranking stands between the fixture and the answer, so
every query of every cell is compared, and the lists come in no order with a count of their own per query.

  test                          cells
  test_route_cell               route {block top-k, select in two steps, select in one run, tile, large k} x metric {L2, inner
                                product, cosine} x element type {fp32, fp16} x dim {below, at, just above a k-step of the scan,
                                several k-steps and a remainder}; each on batches of 1 and 8 (direct routes) or 9 and 40 queries, on
                                exact and gaussian rows (cosine: gaussian), each with five variants on one index and one context:
                                plain, an exclusion with a whole probed list in it, a radius between two scores, a radius above
                                every score, a max_scan_count that ends some probe walks early
  test_raw_rows_shortcut        fp32 dim 32: the direct routes with the query rows at a 16-byte aligned pointer (read unprepared) and
                                at that pointer + 4 bytes (through prep_queries): same bits
  test_coarse_pass_alone        zvec_hip_ivf_coarse_dev against the fp64 ranking of centroids that are untied by construction
  test_probes_from_coarse_dev   coarse_dev -> search_probes_dev == search_dev bit for bit, per route and metric, with an exclusion
  test_refusals                 the documented codes; nothing to read back afterwards

After every search the route the host dispatched is asserted (zvec_hip_ctx_last_ivf_plan); on the tile route the plan arrays are
compared with ivf_plan_ref.plan of the given lists; on every route but large-k last_stats with the probe rule.  Exact rows: counts
and scores bit for bit, every key a distinct admitted row of a probed list with exactly the reported score, on the direct routes
in the reference's order among equal scores.  Gaussian rows: the bands of DESIGN §4 (seed_ref.bands), the key sets equal wherever
the fp64 gap behind the k-th place is wider than twice the select band.  tests/test_ivf_routes_reference_cpu.py shows what these
cells catch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_plan_ref as P  # noqa: E402
import ivf_routes_ref as R  # noqa: E402
import seed_ref as S  # noqa: E402
from test_gpu_ivf_plan import KEY_ADD, KEY_MUL, _check_plan  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NO_READY, NO_INDEX_LOADED, NO_TRAINED = -31, -12, -21, -204, -205
FLT_MAX = 3.4028234663852886e38


def _load(ix):
    import zvec_amd as zv
    se = zv.HipIVFSearcher(ix["dim"], ix["metric"], dtype=ix["dtype"])
    n = ix["vecs"].shape[0]
    assert se.load(ix["cent"], P.list_offsets(ix["sizes"]).astype(np.uint64), ix["vecs"], P.keys_for(n)) == 0
    assert se.info() == (n, ix["nlist"])
    return se


@pytest.fixture(scope="module")
def loaded():
    """(metric, dtype, d, kind) -> (fixture, searcher, context): one index and one context for all the variants of its cells"""
    cache = {}

    def get(metric, dtype, d, kind):
        key = (metric, dtype, d, kind)
        if key not in cache:
            ix = R.index(metric, dtype, d, kind)
            se = _load(ix)
            cache[key] = (ix, se, se.create_context())
        return cache[key]
    yield get
    cache.clear()


def _outputs(nq, k):
    import torch
    return (torch.zeros((nq, k), dtype=torch.int64, device="cuda"), torch.zeros((nq, k), dtype=torch.float32, device="cuda"),
            torch.zeros(nq, dtype=torch.int32, device="cuda"))


def _host(keys, scores, counts):
    return keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.int64)


def _dev_queries(se, q, shift=False):
    """the query rows on the device; shift: the same rows 4 bytes behind an aligned pointer"""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(q, se.np_dtype).reshape(-1))
    if not shift:
        dq = flat.cuda()
        assert dq.data_ptr() % 16 == 0
        return dq, dq.data_ptr()
    assert flat.element_size() == 4
    buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device="cuda")
    buf[1:1 + flat.numel()] = flat.cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4


def _search_probes(se, ctx, q, ids, cnt, k, nprobe, max_scan=R.NO_LIMIT, excluded=None, radius=None, shift=False):
    import torch
    hold, qptr = _dev_queries(se, q, shift)
    nq = len(q)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda()
    d_cnt = torch.from_numpy(np.ascontiguousarray(cnt, np.int32)).cuda()
    out = _outputs(nq, k)
    dex = None if excluded is None else torch.from_numpy(P.pack_bits(excluded).view(np.int64)).cuda()
    torch.cuda.synchronize()
    rc = se.search_probes_dev(qptr, nq, k, nprobe, max_scan, d_ids.data_ptr(), d_cnt.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                              out[2].data_ptr(), ctx, threshold=FLT_MAX if radius is None else radius,
                              d_exclude=None if dex is None else dex.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    del hold
    return _host(*out)


def _positions(ix, keys, what):
    kq = keys.astype(np.int64) - KEY_ADD
    n = ix["vecs"].shape[0]
    assert (kq % KEY_MUL == 0).all() and (kq >= 0).all() and (kq < n * KEY_MUL).all(), "%s: not keys of this index" % what
    return kq // KEY_MUL


def _check_exact(ix, q, ref, got, excluded, ordered, what):
    """counts and scores bit for bit; every key a distinct admitted row of a probed list whose exact score is the reported one;
    ordered (direct routes): the very rows of the reference, equal scores by probe rank, then place in the list"""
    keys, scores, counts = got
    offs = P.list_offsets(ix["sizes"])
    assert np.array_equal(counts, ref["counts"]), "%s: counts %r, reference %r" % (what, counts, ref["counts"])
    for i in range(len(q)):
        c = int(ref["counts"][i])
        want = ref["scores"][i, :c].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref["scores"][i, :c])                 # (exact in fp32: the fixture's promise)
        assert np.array_equal(scores[i, :c].view(np.uint32), want.view(np.uint32)), "%s query %d: scores\n gpu %r\n ref %r" % (
            what, i, scores[i, :c], want)
        pos = _positions(ix, keys[i, :c], "%s query %d" % (what, i))
        assert np.unique(pos).size == c, "%s query %d: a row twice" % (what, i)
        lists = np.searchsorted(offs, pos, side="right") - 1
        assert set(lists.tolist()) <= set(ref["probed"][i]), "%s query %d: a row of a list that was not probed" % (what, i)
        assert excluded is None or not excluded[pos].any(), "%s query %d: an excluded row" % (what, i)
        assert np.array_equal(R.scores64(ix["metric"], ix["vecs"][pos], q[i], ix["d"]), ref["scores"][i, :c]), \
            "%s query %d: a key with another score" % (what, i)
        if ordered:
            assert np.array_equal(pos, ref["pos"][i, :c]), "%s query %d: order among equal scores\n gpu %r\n ref %r" % (
                what, i, pos, ref["pos"][i, :c])


def _check_band(ix, q, ref, got, what):
    """the tolerances of DESIGN §4 on every query; the key sets equal where the k-th place is decided beyond twice the select band"""
    keys, scores, counts = got
    assert np.array_equal(counts, ref["counts"]), "%s: counts %r, reference %r" % (what, counts, ref["counts"])
    wk = P.keys_for(ix["vecs"].shape[0])[np.maximum(ref["pos"], 0)]
    d, nq = ix["d"], len(q)
    bn = np.zeros(nq)
    b64 = np.asarray(ix["vecs"], np.float64)[:, :d]
    for i in range(nq):                                       # per query the largest |b|^2 among the rows either side returned
        c = int(counts[i])
        p = np.unique(np.concatenate([_positions(ix, keys[i, :c], what), ref["pos"][i, :c]]))
        bn[i] = (b64[p] ** 2).sum(1).max() if p.size else 0.0
    kw, band = S.bands(bn, np.asarray(q, np.float64)[:, :d], ix["metric"])
    worst = 0.0
    for i in range(nq):
        c = int(counts[i])
        if c:
            worst = max(worst, float(np.abs(scores[i, :c].astype(np.float64) - ref["scores"][i, :c]).max()))
    print("%s: largest |gpu - fp64| by rank %.3e, smallest band %.3e" % (what, worst, float(band.min()) if nq else 0.0))
    U.tie_tolerant_compare(keys, scores, counts, wk, ref["scores"].astype(np.float32), ref["counts"], what=what, **kw)
    for i in np.nonzero(ref["gap"] > 2.0 * band)[0]:
        c = int(counts[i])
        assert set(keys[i, :c].tolist()) == set(wk[i, :c].tolist()), "%s query %d: key set (gap %r, band %r)" % (what, i, ref["gap"][i], band[i])


def _check_search(ix, se, ctx, c, route, args, got, what):
    """everything one search is held to: route, plan (tile), statistics (all but large k), answer"""
    nq, k, nprobe, q, ids, cnt = c["nq"], c["k"], c["nprobe"], c["q"], c["ids"], c["cnt"]
    plan = ctx.last_ivf_plan()
    want_route = P.expected_route(nq, k, nprobe, ix["sizes"])
    assert plan["route"] == want_route == R.ROUTES[route][0], "%s: route %d, expected %d" % (what, plan["route"], want_route)
    ref = R.answer(ix, q, ids, cnt, k, **args)
    max_scan = args.get("max_scan", R.NO_LIMIT)
    if want_route == P.ROUTE_TILE:
        ltpc = P.level_tpc(P.list_levels(ix["sizes"]), plan["tpc"])
        pl = P.plan([ids[i, :cnt[i]] for i in range(nq)], ix["sizes"], max_scan, ltpc)
        assert [list(p) for p in pl["probed"]] == ref["probed"]
        _check_plan(dict(queries=q, nlist=ix["nlist"], sizes=ix["sizes"]), plan, pl, nprobe, what)
    else:
        assert "slot_begin" not in plan, what
    if want_route != P.ROUTE_LARGE_K:                          # (the large-k route keeps no per-query statistics)
        scanned, probes = se.last_stats(ctx, nq)
        assert np.array_equal(probes.astype(np.int64), [len(p) for p in ref["probed"]]), "%s: probes" % what
        assert np.array_equal(scanned.astype(np.int64), ref["scanned"]), "%s: scanned" % what
    if ix["kind"] == "exact":
        _check_exact(ix, q, ref, got, args.get("excluded"), route in R.DIRECT, what)
    else:
        _check_band(ix, q, ref, got, what)


CELLS = [(route, m, t, d) for route in R.ROUTES for m in R.METRICS for t in R.DTYPES for d in R.DIMS[t]]


@pytest.mark.parametrize("route,metric,dtype,d", CELLS)
def test_route_cell(loaded, route, metric, dtype, d):
    for kind in R.kinds_of(metric):
        ix, se, ctx = loaded(metric, dtype, d, kind)
        for batch in (0, 1):
            c = R.case(ix, route, batch)
            for name in R.VARIANTS:
                args = c["variants"][name]
                what = "%s %s %d queries k %d %s" % (ix["name"], route, c["nq"], c["k"], name)
                got = _search_probes(se, ctx, c["q"], c["ids"], c["cnt"], c["k"], c["nprobe"], **args)
                _check_search(ix, se, ctx, c, route, args, got, what)


@pytest.mark.parametrize("metric", (R.L2, R.IP))
@pytest.mark.parametrize("route", R.DIRECT)
def test_raw_rows_shortcut(loaded, route, metric):
    """fp32 dim 32, no norm slot: an aligned query pointer is read in place by the direct route, the same rows 4 bytes further on go
    through prep_queries — identical outputs, the same route, and both held to the reference"""
    dtype, d = R.RAW_ROWS
    for kind in R.kinds_of(metric):
        ix, se, ctx = loaded(metric, dtype, d, kind)
        assert ix["dim"] == d and d % R.KSTEP[dtype] == 0
        for batch in (0, 1):
            c = R.case(ix, route, batch)
            for name in ("plain", "exclusion", "radius"):
                args = c["variants"][name]
                what = "raw rows %s %s %d queries %s" % (ix["name"], route, c["nq"], name)
                a = _search_probes(se, ctx, c["q"], c["ids"], c["cnt"], c["k"], c["nprobe"], **args)
                ra = ctx.last_ivf_plan()["route"]
                b = _search_probes(se, ctx, c["q"], c["ids"], c["cnt"], c["k"], c["nprobe"], shift=True, **args)
                _check_search(ix, se, ctx, c, route, args, b, what + " (shifted)")
                assert ra == ctx.last_ivf_plan()["route"], what
                assert np.array_equal(a[2], b[2]), what
                for i in range(c["nq"]):
                    n = int(a[2][i])
                    assert np.array_equal(a[0][i, :n], b[0][i, :n]) and np.array_equal(a[1][i, :n].view(np.uint32), b[1][i, :n].view(np.uint32)), \
                        "%s query %d: the aligned and the shifted rows answer differently" % (what, i)


# ---- the coarse pass alone ---------------------------------------------------------------------------------------------------------------
def _coarse_index(metric, dtype, cent, d, sizes, kind_rows=None):
    import zvec_amd as zv
    rng = np.random.default_rng(3)
    n = int(np.sum(sizes))
    x = rng.integers(1, 8, (n, d)).astype(np.float32) if kind_rows is None else kind_rows
    vecs = R.cosine_rows(x, dtype) if metric == R.COS else x.astype(R.NP_DTYPE[dtype])
    se = zv.HipIVFSearcher(cent.shape[1], metric, dtype=dtype)
    assert se.load(cent, P.list_offsets(sizes).astype(np.uint64), vecs, P.keys_for(n)) == 0
    return se, vecs


def _coarse(se, ctx, q, nprobe, nlist):
    import torch
    hold, qptr = _dev_queries(se, q)
    nq, np_ = len(q), min(nprobe, nlist)
    d_ids = torch.full((nq, np_), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert se.coarse_dev(qptr, nq, nprobe, d_ids.data_ptr(), d_cnt.data_ptr(), ctx) == 0
    torch.cuda.synchronize()
    del hold
    return d_ids, d_cnt


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("metric", R.METRICS)
def test_coarse_pass_alone(metric, dtype):
    """[count][min(nprobe, nlist)] ids in coarse-score order and the counts, exactly the fp64 ranking; nothing to read back after"""
    nlist = R.COARSE_NLIST
    se = ctx = None
    for nq in (1, 8, 9, 40):
        cent, q, d = R.coarse_fixture(metric, dtype, nq)
        if se is None:                                        # (the centroids do not depend on the batch)
            se, _ = _coarse_index(metric, dtype, cent, d, np.full(nlist, 3))
            ctx = se.create_context()
        order, _ = R.coarse_ranking(metric, cent, q, d)
        for nprobe in (1, 3, nlist, nlist + 5):
            what = "coarse %s %s %d queries nprobe %d" % (metric, dtype, nq, nprobe)
            d_ids, d_cnt = _coarse(se, ctx, q, nprobe, nlist)
            np_ = min(nprobe, nlist)
            assert np.array_equal(d_cnt.cpu().numpy(), np.full(nq, np_)), what
            assert np.array_equal(d_ids.cpu().numpy().astype(np.int64), order[:, :np_]), what
            assert ctx.last_ivf_plan()["route"] == P.ROUTE_NONE, what


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("route", list(R.ROUTES))
def test_probes_from_coarse_dev(route, metric):
    """what the header promises: coarse_dev's lists fed to search_probes_dev give what search_dev gives for the same arguments — keys,
    scores, counts, route and statistics, bit for bit — with and without an exclusion (centroids untied by construction, so the two
    coarse kernels rank alike; a scan limit that ends some probe walks early)"""
    import torch
    _, nprobe, batches = R.ROUTES[route]
    nq, k = batches[1]
    cent, q, d = R.coarse_fixture(metric, "fp32", nq, nlist=R.NLIST, step=0.125)
    rows = None if metric != R.COS else np.random.default_rng(8).standard_normal((int(R.SIZES.sum()), d)).astype(np.float32)
    se, _ = _coarse_index(metric, "fp32", cent, d, R.SIZES, rows)
    ctx = se.create_context()
    max_scan = 300
    for excluded in (None, P.exclusion(int(R.SIZES.sum()))):
        what = "%s %s%s" % (route, metric, "" if excluded is None else " excluded")
        dex = None if excluded is None else torch.from_numpy(P.pack_bits(excluded).view(np.int64)).cuda()
        ex = None if dex is None else dex.data_ptr()
        hold, qptr = _dev_queries(se, q)
        a = _outputs(nq, k)
        torch.cuda.synchronize()
        assert se.search_dev(qptr, nq, k, nprobe, max_scan, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), ctx, d_exclude=ex) == 0
        torch.cuda.synchronize()
        route_a = ctx.last_ivf_plan()["route"]
        stats_a = se.last_stats(ctx, nq) if route_a != P.ROUTE_LARGE_K else None
        assert route_a == P.expected_route(nq, k, nprobe, R.SIZES) == R.ROUTES[route][0], what
        d_ids, d_cnt = _coarse(se, ctx, q, nprobe, R.NLIST)
        order, _ = R.coarse_ranking(metric, cent, q, d)
        assert np.array_equal(d_ids.cpu().numpy().astype(np.int64), order[:, :nprobe]), what
        b = _outputs(nq, k)
        assert se.search_probes_dev(qptr, nq, k, nprobe, max_scan, d_ids.data_ptr(), d_cnt.data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                    b[2].data_ptr(), ctx, d_exclude=ex) == 0
        torch.cuda.synchronize()
        assert ctx.last_ivf_plan()["route"] == route_a, what
        if stats_a is not None:
            stats_b = se.last_stats(ctx, nq)
            assert np.array_equal(stats_a[0], stats_b[0]) and np.array_equal(stats_a[1], stats_b[1]), what
            rule = [P.probe_rule(order[i, :nprobe], R.SIZES, max_scan) for i in range(nq)]
            assert np.array_equal(stats_b[1], [len(r[0]) for r in rule]) and np.array_equal(stats_b[0], [r[1] for r in rule]), what
            assert nprobe == 2 or (stats_b[1] < nprobe).any(), what                           # the scan limit is at work
        ha, hb = _host(*a), _host(*b)
        assert np.array_equal(ha[2], hb[2]) and (ha[2] > 0).all(), what
        for i in range(nq):
            n = int(ha[2][i])
            assert np.array_equal(ha[0][i, :n], hb[0][i, :n]), "%s query %d: keys" % (what, i)
            assert np.array_equal(ha[1][i, :n].view(np.uint32), hb[1][i, :n].view(np.uint32)), "%s query %d: scores" % (what, i)
        del hold


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _nothing_to_read(se, ctx, nq, what):
    from zvec_amd import _lib
    assert ctx.last_ivf_plan()["route"] == P.ROUTE_NONE, what
    with pytest.raises(_lib.ZvecHipError) as e:
        se.last_stats(ctx, nq)
    assert e.value.code == NO_READY, what


def test_refusals():
    """the codes the entry points document; a refused call is no search: the context it was given has nothing to read back"""
    import torch
    import zvec_amd as zv
    from zvec_amd import _lib
    cent, q, d = R.coarse_fixture(R.L2, "fp32", 4)
    nlist, nq, k = R.COARSE_NLIST, 4, 5
    se, _ = _coarse_index(R.L2, "fp32", cent, d, np.full(nlist, 3))
    hold, qptr = _dev_queries(se, q)
    d_ids = torch.zeros((nq, 3), dtype=torch.int32, device="cuda")
    d_cnt = torch.full((nq,), 3, dtype=torch.int32, device="cuda")
    out = _outputs(nq, k)
    outs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    torch.cuda.synchronize()
    for what, ids, cnt in (("no probe ids", 0, d_cnt.data_ptr()), ("no probe counts", d_ids.data_ptr(), 0)):
        ctx = se.create_context()
        assert se.search_probes_dev(qptr, nq, k, 3, R.NO_LIMIT, ids, cnt, *outs, ctx) == INVALID, what
        _nothing_to_read(se, ctx, nq, what)
        assert se.coarse_dev(qptr, nq, 3, ids, cnt, ctx) == INVALID, what
        _nothing_to_read(se, ctx, nq, what)
    ctx = se.create_context()
    assert se.search_probes_dev(qptr, nq, 0, 3, R.NO_LIMIT, d_ids.data_ptr(), d_cnt.data_ptr(), *outs, ctx) == INVALID
    _nothing_to_read(se, ctx, nq, "topk 0")
    # before load
    empty = zv.HipIVFSearcher(d, R.L2)
    ctx = empty.create_context()
    assert empty.search_probes_dev(qptr, nq, k, 3, R.NO_LIMIT, d_ids.data_ptr(), d_cnt.data_ptr(), *outs, ctx) == NO_INDEX_LOADED
    _nothing_to_read(empty, ctx, nq, "search before load")
    assert empty.coarse_dev(qptr, nq, 3, d_ids.data_ptr(), d_cnt.data_ptr(), ctx) == NO_TRAINED
    _nothing_to_read(empty, ctx, nq, "coarse pass before load")
    # the same calls are served (so the refusals above were about what they name) ...
    ctx = se.create_context()
    assert se.coarse_dev(qptr, nq, 3, d_ids.data_ptr(), d_cnt.data_ptr(), ctx) == 0
    assert se.search_probes_dev(qptr, nq, k, 3, R.NO_LIMIT, d_ids.data_ptr(), d_cnt.data_ptr(), *outs, ctx) == 0
    torch.cuda.synchronize()
    assert ctx.last_ivf_plan()["route"] == P.ROUTE_DIRECT_SELECT
    # ... until the centroids stand in a space of their own: the coarse pass alone has no queries of that space
    ccent = np.ascontiguousarray(np.random.default_rng(1).standard_normal((nlist, d + 4)).astype(np.float32))
    assert _lib.lib().zvec_hip_ivf_set_coarse_space(se._h, d + 4, 0, ccent.ctypes.data_as(C.c_void_p), nlist) == 0
    ctx = se.create_context()
    assert se.coarse_dev(qptr, nq, 3, d_ids.data_ptr(), d_cnt.data_ptr(), ctx) == UNSUPPORTED
    _nothing_to_read(se, ctx, nq, "coarse pass on a separate coarse space")
    torch.cuda.synchronize()
    del hold

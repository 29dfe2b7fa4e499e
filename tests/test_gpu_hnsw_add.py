"""Appending rows to an HNSW graph on the GPU (zvec_hip_hnsw_add*, _reserve, _last_add_info), against the model of
tests/hnsw_add_ref.py and the three consequences of DESIGN §3c "Appending".  Every row set but the last is integer-valued, so every fp32
distance is exact in any summation order: the exported graph equals the model's array for array after every call, and the four
counters of every call equal the model's.  On Gaussian rows the graph is checked for validity and for the recall a search reaches."""
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
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, OUT_OF_RANGE, NOREADY, INVALID = -12, -17, -21, -31
NAMES = {"l2": "SquaredEuclidean", "ip": "InnerProduct"}
OPTIONS = {"hnsw_build_round_div": 16, "hnsw_build_round_max": 4096, "hnsw_ws_bytes": 1 << 30}
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


def _params(p):
    return dict(m=p.m, m0=p.m0, ef_construction=p.ef_construction, prune_cnt=p.prune_cnt, min_neighbors=p.min_neighbors,
                scaling_factor=p.scaling_factor)


def _searcher(fx):
    import zvec_amd as zv
    return zv.HipHnswSearcher(fx.rows.shape[1], NAMES[fx.metric])


def _same_graph(se, g, what=""):
    i = se.info()
    n = g.rows.shape[0]
    assert (i["n"], i["m0"], i["max_level"], i["entry_point"]) == (n, g.m0, g.max_level, g.entry_point), what
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    assert np.array_equal(keys, g.keys), what
    assert np.array_equal(cnt0, g.cnt0), what
    assert np.array_equal(nbr0, g.nbr0), what
    if g.max_level > 0:
        assert (i["m"], i["n_upper"]) == (g.m, g.n_upper), what
        assert np.array_equal(upper_of, g.upper_of) and np.array_equal(cnt_up, g.cnt_up) and np.array_equal(nbr_up, g.nbr_up), what
    else:
        assert upper_of is None, what
    assert np.array_equal(se.get_vectors_by_ids(np.arange(n)), g.rows), what


def _counters(info):
    return B.Counters(info["rounds"], info["dists"], info["requests"], info["prunes"])


def _run(fx, calls, se=None, first_is_build=True, dev=False, ws_bytes=1 << 30, after=None, explicit=False):
    """the fixture's calls on a handle: the first as a build (or an add on the empty handle), the others as adds; after(j, se) runs
    behind call j.  Returns the handle and the info of every call."""
    se = se or _searcher(fx)
    kw = _params(fx.params)
    infos = []
    keys = _keys(fx.rows.shape[0])
    with _options(hnsw_build_round_div=fx.round_div, hnsw_build_round_max=fx.round_max):
        for j, k in enumerate(calls):
            a, e = k.first, k.first + k.count
            if j == 0 and first_is_build:
                assert se.build(fx.rows[a:e], keys=keys[a:e], levels=fx.levels[a:e], **kw) == 0
                infos.append(se.build_info())
            else:
                with _options(hnsw_ws_bytes=ws_bytes):
                    args = dict(keys=keys[a:e], levels=fx.levels[a:e], **(kw if explicit or j == 0 else {}))
                    if dev:
                        import torch
                        d = torch.from_numpy(fx.rows[a:e]).to(torch.device("cuda:0"))
                        torch.cuda.synchronize()
                        assert se.add_dev(d.data_ptr(), k.count, **args) == 0
                    else:
                        assert se.add(fx.rows[a:e], **args) == 0
                infos.append(se.add_info())
                assert (infos[-1]["first"], infos[-1]["count"]) == (a, k.count)
            if after is not None:
                after(j, se)
    return se, infos


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_p1_sequential_rounds_do_not_see_the_cuts(metric):
    """round_div 0: build(100), then adds of 1, 7, 64 and the rest give the graph and the summed counters of one build of all rows"""
    fx = B.base(metric, 0, 64)
    g, c = B.build_model(fx.rows, fx.params, fx.levels, 0, 64, metric, keys=_keys(600))
    fxa = A.Fixture(fx.rows, fx.params, fx.levels, (100, 1, 7, 64, 428), 0, 64, metric)
    calls = [A.Call(a, k, None, None, None, None) for a, k in zip((0, 100, 101, 108, 172), fxa.calls)]
    se, infos = _run(fxa, calls)
    _same_graph(se, g, "p1 " + metric)
    total = B.Counters(*[sum(_counters(i)[k] for i in infos) for k in range(4)])
    print("gpu", tuple(total), "model", tuple(c))
    assert total == c
    assert all(i["rounds_one"] == i["rounds"] for i in infos[1:])
    assert (infos[-1]["top"], infos[-1]["entry_point"]) == (g.max_level, g.entry_point)
    b = se.build_info()
    assert _counters(b) == _counters(infos[0])            # last_build_info keeps describing the build


def test_p2_one_row_per_call_from_an_empty_handle():
    fx = B.base("l2", 16, 64)
    n = 150
    g, c = B.build_model(fx.rows[:n], fx.params, fx.levels[:n], 0, 64, "l2", keys=_keys(n))
    fxa = A.Fixture(fx.rows[:n], fx.params, fx.levels[:n], (1,) * n, 16, 64, "l2")
    calls = [A.Call(i, 1, None, None, None, None) for i in range(n)]
    se, infos = _run(fxa, calls, first_is_build=False)
    _same_graph(se, g, "p2")
    assert B.Counters(*[sum(_counters(i)[k] for i in infos) for k in range(4)]) == c
    assert infos[0]["rounds"] == 0 and all(i["rounds"] == 1 and i["rounds_one"] == 1 for i in infos[1:])


@pytest.mark.parametrize("name", list(A.FIXTURES))
def test_p3_every_call_equals_the_model(name):
    """cuts inside a round; a level-3 node inside a call and a level-2 node at the head of one (stride 1 -> 3); upper arrays made by
    an add; appended nodes pruning old links; lists wider than a wave on both reverse paths; more than 1024 nodes before the add;
    inner product"""
    fx, calls = A.model_of(name)

    def after(j, se):
        _same_graph(se, calls[j].graph, "%s after call %d" % (name, j))

    se, infos = _run(fx, calls, after=after)
    for j, (k, i) in enumerate(zip(calls, infos)):
        print(name, j, "gpu", tuple(_counters(i)), "model", tuple(k.counters))
        assert _counters(i) == k.counters, (name, j)
        if j:
            assert bool(i["restrided"]) == k.restrided, (name, j)
            assert i["rounds_one"] == k.book["one_rounds"], (name, j)
            assert (i["top"], i["entry_point"]) == (k.graph.max_level, k.graph.entry_point)
    if name == "first_upper":
        assert se.export()[3] is not None and se.info()["n_upper"] == 4


def test_growth_and_reserve():
    fx, calls = A.model_of("cut")
    se, infos = _run(fx, calls)
    assert any(i["grew_rows"] for i in infos[1:]) and any(i["grew_upper"] for i in infos[1:])
    assert all(i["cap_rows"] >= k.first + k.count for i, k in zip(infos[1:], calls[1:]))
    caps = []

    def after(j, se2):
        if j == 0:
            assert se2.reserve(600) == 0
            assert se2.reserve(10) == 0                                     # never shrinks
            _same_graph(se2, calls[0].graph, "after reserve")
        else:
            caps.append((se2.add_info()["cap_rows"], se2.add_info()["cap_upper"]))

    se2, infos2 = _run(fx, calls, after=after)
    assert not any(i["grew_rows"] or i["grew_upper"] for i in infos2[1:])
    assert len(set(caps)) == 1 and caps[0][0] == 600 and caps[0][1] >= calls[-1].graph.n_upper
    _same_graph(se2, calls[-1].graph, "reserved")
    _same_graph(se, calls[-1].graph, "grown")
    # a reserve on an empty handle is kept for the first add
    se3 = _searcher(fx)
    assert se3.reserve(600, 300) == 0
    se3, infos3 = _run(fx, calls, se=se3, first_is_build=False)
    assert (infos3[0]["cap_rows"], infos3[0]["cap_upper"]) == (600, 300)
    assert not any(i["grew_rows"] or i["grew_upper"] for i in infos3[1:])
    _same_graph(se3, calls[-1].graph, "reserved before the first add")


def test_add_dev_equals_add():
    fx, calls = A.model_of("top_raised")
    se, infos = _run(fx, calls, dev=True)
    _same_graph(se, calls[-1].graph, "add_dev")
    assert [_counters(i) for i in infos] == [k.counters for k in calls]


def test_add_to_a_loaded_graph():
    """the model's graph of the first 200 rows through load, then adds with explicit parameters"""
    fx, calls = A.model_of("cut")
    g = calls[0].graph
    se = _searcher(fx)
    assert se.load(g.rows, g.nbr0, g.cnt0, g.entry_point, keys=g.keys, upper_of=g.upper_of, nbr_up=g.nbr_up, cnt_up=g.cnt_up) == 0
    with pytest.raises(Exception):
        se.add_info()
    with _options(hnsw_build_round_div=fx.round_div, hnsw_build_round_max=fx.round_max):
        for k in calls[1:]:
            a, e = k.first, k.first + k.count
            assert se.add(fx.rows[a:e], keys=_keys(600)[a:e], levels=fx.levels[a:e], **_params(fx.params)) == 0
            assert _counters(se.add_info()) == k.counters
            _same_graph(se, k.graph, "loaded, call at %d" % a)
    with pytest.raises(Exception):
        se.build_info()                                                     # nothing was built on this handle


def test_add_on_an_empty_handle_equals_build():
    fx, g, c, _ = B.model_of("l2-div16-max64")
    fxa = A.Fixture(fx.rows, fx.params, fx.levels, (600,), fx.round_div, fx.round_max, fx.metric)
    se, infos = _run(fxa, [A.Call(0, 600, None, None, None, None)], first_is_build=False)
    _same_graph(se, g._replace(keys=_keys(600)), "add on empty")
    assert _counters(infos[0]) == c and infos[0]["restrided"] == 1 and infos[0]["grew_rows"] == 1
    assert se.add(np.zeros((0, 24), np.float32)) == 0                       # count == 0 changes nothing
    assert se.add_info() == infos[0]
    _same_graph(se, g._replace(keys=_keys(600)), "after an add of no rows")


def test_add_after_a_build_of_no_rows_equals_build():
    """a handle that built zero rows holds no nodes: the add is the build of its rows, and build_info keeps the empty build"""
    fx, g, c, _ = B.model_of("l2-div16-max64")
    fxa = A.Fixture(fx.rows, fx.params, fx.levels, (600,), fx.round_div, fx.round_max, fx.metric)
    se = _searcher(fx)
    assert se.add(np.zeros((0, 24), np.float32)) == 0                       # no rows on a fresh handle: nothing happens
    with pytest.raises(Exception):
        se.add_info()
    assert se.info()["n"] == 0
    # (no levels are passed for no rows, so the build asks for a scaling_factor levels could be generated with)
    assert se.build(np.zeros((0, 24), np.float32), **dict(_params(fx.params), scaling_factor=5)) == 0
    empty = se.build_info()
    assert (empty["rounds"], empty["dists"], empty["requests"], empty["prunes"]) == (0, 0, 0, 0)
    se, infos = _run(fxa, [A.Call(0, 600, None, None, None, None)], se=se, first_is_build=False)
    _same_graph(se, g._replace(keys=_keys(600)), "add after a build of no rows")
    assert _counters(infos[0]) == c and infos[0]["restrided"] == 1 and infos[0]["grew_rows"] == 1
    assert se.build_info() == empty


def _grow(cap, need, reserved):
    """hnsw_grow (host/hnsw_add_plan.h)"""
    return cap if need <= cap else max(need, reserved, 2 * cap)


def test_a_build_keeps_exact_capacity_even_after_a_reserve():
    """build(200) leaves room for 200 rows and its own upper nodes, whatever a reserve said before; the add of one row shows it"""
    fx = B.base("l2", 16, 64)
    lv = fx.levels
    nu0, nu1 = int((lv[:200] >= 1).sum()), int((lv[:201] >= 1).sum())
    assert nu0 > 0
    for reserve, want_rows, want_upper in ((False, 0, 0), (True, 600, min(600, 600 // 49 + 64))):      # (no build yet: scaling_factor 50)
        se = _searcher(fx)
        if reserve:
            assert se.reserve(600) == 0
        with _options(hnsw_build_round_div=fx.round_div, hnsw_build_round_max=fx.round_max):
            assert se.build(fx.rows[:200], levels=lv[:200], **_params(fx.params)) == 0
            assert se.add(fx.rows[200:201], levels=lv[200:201]) == 0
        i = se.add_info()
        assert (i["grew_rows"], i["cap_rows"]) == (1, _grow(200, 201, want_rows)) and i["cap_rows"] == (600 if reserve else 400)
        cap_upper = _grow(nu0, nu1, want_upper)
        assert (i["grew_upper"], i["cap_upper"]) == (int(cap_upper > nu0), cap_upper)
        if lv[200] == 0:
            assert (i["grew_upper"], i["cap_upper"]) == (0, nu0)


def test_generated_levels_do_not_depend_on_the_calls():
    import zvec_amd as zv
    fx = B.base()
    p = B.params(m=8, m0=16, ef_construction=16)
    lv = B.levels_model(600, 8, 5)
    calls = A.add_model(fx.rows, p, lv, (300, 1, 299), 16, 64, "l2")
    se = zv.HipHnswSearcher(24)
    with _options(hnsw_build_round_div=16, hnsw_build_round_max=64):
        assert se.build(fx.rows[:300], m=8, m0=16, ef_construction=16, seed=5) == 0
        assert se.add(fx.rows[300:301]) == 0                               # NULL parameters: the build's, its seed included
        assert se.add(fx.rows[301:], seed=5) == 0
    _same_graph(se, calls[-1].graph, "generated levels")


def test_slices_are_invisible():
    fx, calls = A.model_of("spill")
    for slices, ws in ((1, 1 << 30), (3, 103776), (17, 17296)):
        assert A.slices_of(fx, 1, ws) == slices
        se, infos = _run(fx, calls, ws_bytes=ws)
        assert infos[1]["slices"] == slices and _counters(infos[1]) == calls[1].counters
        _same_graph(se, calls[1].graph, "%d slices" % slices)


def test_searches_between_calls():
    fx, calls = A.model_of("cut")
    q = H.exact_queries(calls[-1].graph, np.random.default_rng(9), 8)
    seen = []

    def after(j, se):
        g = calls[j].graph
        n = g.rows.shape[0]
        ctx = se.create_context()
        ctx.set_topk(10)
        assert se.search(q, 8, ctx, 16) == 0
        scanned, hops, _ = se.last_stats(ctx, 8)
        for i in range(8):
            r = H.search_model(g, q[i], 10, 16, metric=fx.metric)
            assert ctx.counts[i] == r.keys.size and np.array_equal(ctx.keys[i, :r.keys.size], r.keys), (j, i)
            assert np.array_equal(ctx.scores[i, :r.keys.size], r.scores) and (scanned[i], hops[i]) == (r.scanned, r.hops), (j, i)
        if j == 1:
            # an exclude bitset sized for the new n that excludes an appended row: the nearest appended row of query 0
            d = H.scores64(g.rows, q[0], fx.metric)
            v = calls[1].first + int(np.argmin(d[calls[1].first:]))
            ex = np.zeros(n, bool)
            ex[v] = True
            plain = H.search_model(g, q[0], 10, 16, metric=fx.metric)
            r = H.search_model(g, q[0], 10, 16, exclude=ex, metric=fx.metric)
            ctx.set_exclude_bitset(H.words_of(ex))
            assert se.search(q[:1], 1, ctx, 16) == 0
            assert np.array_equal(ctx.keys[0, :r.keys.size], r.keys) and g.keys[v] not in ctx.keys[0]
            seen.append(g.keys[v] in plain.keys)

    _run(fx, calls, after=after)
    assert seen == [True]                                                  # without the bitset the appended row is an answer


def test_refusals_leave_the_graph_alone():
    from zvec_amd import _lib
    fx, calls = A.model_of("top_raised")
    se, _ = _run(fx, calls[:1])
    g = calls[0].graph
    rows = fx.rows[150:160]
    lv = np.zeros(10, np.uint32)
    before = se.info()

    def untouched(rc, want):
        assert rc == want
        assert se.info() == before
        _same_graph(se, g, "after a refusal")
        with pytest.raises(Exception):
            se.add_info()                                                   # no add has succeeded yet

    untouched(se.add(rows, levels=lv, m0=16), INVALID)
    untouched(se.add(rows, levels=lv, m=8), INVALID)
    bad = lv.copy()
    bad[5] = 16
    untouched(se.add(rows, levels=bad), INVALID)
    untouched(se.add(rows, levels=lv, ef_construction=513), UNSUPPORTED)
    untouched(se.add(rows, levels=lv, min_neighbors=5), INVALID)
    L = _lib.lib()
    untouched(L.zvec_hip_hnsw_add(se._h, 10, None, None, None, C.c_void_p(lv.ctypes.data)), INVALID)
    untouched(L.zvec_hip_hnsw_add(se._h, 0xfffffff0, C.c_void_p(rows.ctypes.data), None, None, None), OUT_OF_RANGE)
    info = _lib.HnswAddInfo()
    assert L.zvec_hip_hnsw_last_add_info(None, C.byref(info)) == INVALID and L.zvec_hip_hnsw_last_add_info(se._h, None) == INVALID
    assert L.zvec_hip_hnsw_reserve(None, 10, 0) == INVALID
    assert L.zvec_hip_hnsw_add(None, 0, None, None, None, None) == INVALID
    assert L.zvec_hip_hnsw_last_add_info(se._h, C.byref(info)) == NOREADY
    assert se.add(rows, levels=lv) == 0 and se.info()["n"] == 160         # and the handle still takes a sound call


def test_quality_on_gaussian_rows():
    """default rounds; the first half built, the second added in four calls; recall@10 at ef 32 is no more than two standard errors
    below the sequential model's (B.QUALITY_P, the floor of tests/test_gpu_hnsw_build.py)"""
    import zvec_amd as zv
    rows, q, levels = B.quality_data()
    p = B.QUALITY_PARAMS
    n = B.QUALITY_N
    se = zv.HipHnswSearcher(B.QUALITY_DIM)
    half = n // 2
    assert se.build(rows[:half], levels=levels[:half], m=p.m, m0=p.m0, ef_construction=p.ef_construction) == 0
    cuts = [half, half + 1, half + 300, half + 650, n]
    for a, e in zip(cuts[:-1], cuts[1:]):
        assert se.add(rows[a:e], levels=levels[a:e]) == 0
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    i = se.info()
    assert i["n"] == n and (cnt0 <= p.m0).all() and (cnt_up <= p.m).all()
    lists = [nbr0[v, :cnt0[v]] for v in range(n)]
    where = [v for v in range(n)]
    for u, v in enumerate(np.nonzero(levels >= 1)[0]):
        assert upper_of[v] == u
        for l in range(i["max_level"]):
            assert l < levels[v] or cnt_up[u, l] == 0
            lists.append(nbr_up[u, l, :cnt_up[u, l]])
            where.append(v)
    for v, x in zip(where, lists):
        assert v not in x and len(set(x.tolist())) == x.size
    for v in range(n):
        assert (nbr0[v, cnt0[v]:] == 0).all()
    H.check_graph(H.Graph(rows, keys, p.m0, nbr0, cnt0, i["max_level"], p.m, i["n_upper"], upper_of, nbr_up, cnt_up, i["entry_point"]))
    ctx = se.create_context()
    ctx.set_topk(B.QUALITY_K)
    assert se.search(q, B.QUALITY_Q, ctx, B.QUALITY_EF) == 0
    got = B.recall(ctx.keys, B.quality_truth(rows, q))
    print("recall@10 %.4f, floor %.4f (p = %.4f)" % (got, B.quality_floor(), B.QUALITY_P))
    assert got >= B.quality_floor()


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_append")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "hnsw_append.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_append ok" in out.stdout.decode()

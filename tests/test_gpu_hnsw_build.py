"""Building an HNSW graph on the GPU (zvec_hip_hnsw_build*), against the model of tests/hnsw_build_ref.py.  Every row set but the last
is integer-valued, so every fp32 distance is exact in any summation order: the exported graph equals the model's array for array,
and the four counters (rounds, distances computed, requests raised, prunes run) equal the model's.  On Gaussian rows fp32 rounding
may reorder near-ties, so the graph is checked for validity and for the recall a search on it reaches."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, NOREADY, INVALID = -12, -21, -31
NAMES = {"l2": "SquaredEuclidean", "ip": "InnerProduct"}
OPTIONS = {"hnsw_build_round_div": 16, "hnsw_build_round_max": 4096, "hnsw_ws_bytes": 1 << 30}


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


def _keys(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


def _build(fx, levels="fixture", dev=False, seed=0, ws_bytes=1 << 30):
    import zvec_amd as zv
    se = zv.HipHnswSearcher(fx.rows.shape[1], NAMES[fx.metric])
    p = fx.params
    lv = fx.levels if isinstance(levels, str) else levels
    n = fx.rows.shape[0]
    kw = dict(keys=_keys(n), levels=lv, m=p.m, m0=p.m0, ef_construction=p.ef_construction, prune_cnt=p.prune_cnt,
              min_neighbors=p.min_neighbors, scaling_factor=p.scaling_factor, seed=seed)
    with _options(hnsw_build_round_div=fx.round_div, hnsw_build_round_max=fx.round_max, hnsw_ws_bytes=ws_bytes):
        if dev:
            import torch
            d = torch.from_numpy(fx.rows).to(torch.device("cuda:0"))
            torch.cuda.synchronize()
            assert se.build_dev(d.data_ptr(), n, **kw) == 0
        else:
            assert se.build(fx.rows, **kw) == 0
    return se


def _same(se, g, c, what=""):
    """the handle holds the model's graph, array for array, and the build counted what the model counted"""
    i = se.info()
    n = g.rows.shape[0]
    assert (i["n"], i["m0"], i["max_level"], i["entry_point"]) == (n, g.m0, g.max_level, g.entry_point), what
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    assert np.array_equal(keys, _keys(n)), what
    assert np.array_equal(cnt0, g.cnt0), what
    assert np.array_equal(nbr0, g.nbr0), what
    if g.max_level > 0:
        assert (i["m"], i["n_upper"]) == (g.m, g.n_upper), what
        assert np.array_equal(upper_of, g.upper_of) and np.array_equal(cnt_up, g.cnt_up) and np.array_equal(nbr_up, g.nbr_up), what
    else:
        assert upper_of is None
    assert np.array_equal(se.get_vectors_by_ids(np.arange(n)), g.rows), what
    b = se.build_info()
    print(what, "gpu", (b["rounds"], b["dists"], b["requests"], b["prunes"]), "model", tuple(c))
    assert (b["rounds"], b["dists"], b["requests"], b["prunes"]) == tuple(c), what
    assert (b["top"], b["entry_point"]) == (g.max_level, g.entry_point), what
    return b


@pytest.mark.parametrize("name", [k for k in B.FIXTURES if k != "sliced"])
def test_exact_rows_equal_the_model(name):
    """L2 and IP under round_div 0 / 1 / 16 and round_max 7 / 64 with level-2 and level-3 nodes mid-sequence; lists wider than a wave;
    every W taken whole; prune_cnt below and above m; min_neighbors = m; dim 5 and 100; duplicate rows; one target asked for more
    links in a round than it holds; 1, 2 and 35 rows"""
    fx, g, c, _ = B.model_of(name)
    _same(_build(fx), g, c, name)


def test_no_rows():
    import zvec_amd as zv
    se = zv.HipHnswSearcher(8)
    with pytest.raises(Exception):
        se.build_info()
    assert se.build(np.zeros((0, 8), np.float32), m=8) == 0
    assert se.info()["n"] == 0
    b = se.build_info()
    assert (b["rounds"], b["dists"], b["requests"], b["prunes"]) == (0, 0, 0, 0)
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search(np.ones((2, 8), np.float32), 2, ctx, 8) == 0 and (ctx.counts == 0).all()


def test_slices_are_invisible():
    """the insert phase of the rounds at 256 and 512 nodes cut into 3 and into 17 slices"""
    fx, g, c, _ = B.model_of("sliced")
    assert _same(_build(fx), g, c, "whole")["slices"] == 1
    for slices, ws in ((3, 6400), (17, 1024)):
        assert B.slices_of(fx, ws) == slices
        assert _same(_build(fx, ws_bytes=ws), g, c, "%d slices" % slices)["slices"] == slices


def test_build_dev_equals_build():
    fx, g, c, _ = B.model_of("dim100")
    _same(_build(fx, dev=True), g, c, "build_dev")


def test_generated_levels():
    fx = B.base()
    fx = fx._replace(params=B.params(m=8, m0=16, ef_construction=16), levels=None)
    lv = B.levels_model(600, 8, 5)
    assert lv.max() >= 2
    g, c = B.build_model(fx.rows, fx.params, lv, fx.round_div, fx.round_max, fx.metric, keys=_keys(600))
    _same(_build(fx, levels=None, seed=5), g, c, "generated")
    import zvec_amd as zv
    assert np.array_equal(zv.hnsw_levels(600, 8, 5), lv)


def test_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    rows = B.base_rows()[:50]
    lv = np.zeros(50, np.uint32)
    se = zv.HipHnswSearcher(24)
    assert se.build(rows, levels=lv, m=4, ef_construction=H_MAX_EF + 1) == UNSUPPORTED
    assert se.build(rows, levels=lv, m=4, m0=257) == UNSUPPORTED
    assert se.build(rows, levels=lv, m=129) == UNSUPPORTED
    assert se.build(rows, levels=lv, m=4, min_neighbors=5) == INVALID
    assert se.build(rows, levels=lv + 16, m=4) == INVALID
    assert se.build(rows, m=4) == INVALID                                  # (generated levels: scaling_factor = m is below 5)
    assert se.build(rows, m=4, scaling_factor=1001) == INVALID
    assert se.info()["n"] == 0                                             # the handle was not touched
    assert se.build(rows, levels=lv, m=128, m0=256, ef_construction=H_MAX_EF) == 0
    h = C.c_void_p()
    assert _lib.lib().zvec_hip_hnsw_create(4097, _lib.DT_FP32, _lib.METRIC_L2, 0, C.byref(h)) == UNSUPPORTED       # dim > HNSW_MAX_DIM
    L = _lib.lib()
    assert L.zvec_hip_set_option(b"hnsw_build_round_max", 0) == INVALID
    assert L.zvec_hip_set_option(b"hnsw_build_round_div", -1) == INVALID
    out = np.zeros(4, np.uint32)
    assert L.zvec_hip_hnsw_build_levels(4, 4, 0, C.c_void_p(out.ctypes.data)) == INVALID


H_MAX_EF = 512


def test_a_refused_build_over_a_graph_changes_nothing():
    """a build replaces the graph only when it succeeds: after two refused builds the handle still holds the first 200 rows of
    the append model's "cut" fixture, its build info, and answers as before"""
    import hnsw_add_ref as A
    fx, calls = A.model_of("cut")
    g, c = calls[0].graph, calls[0].counters
    n = g.rows.shape[0]
    first = B.Fixture(fx.rows[:n], fx.params, fx.levels[:n], fx.round_div, fx.round_max, fx.metric)
    se = _build(first)
    before = (se.info(), se.build_info(), se.export())
    bad = fx.levels[:n].copy()
    bad[n // 2] = 16
    p = fx.params
    assert se.build(fx.rows[:n], levels=bad, m=p.m, m0=p.m0, ef_construction=p.ef_construction) == INVALID
    assert se.build(fx.rows[:n], levels=fx.levels[:n], m=p.m, m0=p.m0, ef_construction=H_MAX_EF + 1) == UNSUPPORTED
    assert (se.info(), se.build_info()) == before[:2]
    for x, y in zip(se.export(), before[2]):
        assert np.array_equal(x, y)
    _same(se, g, c, "after two refused builds")
    q = H.exact_queries(g, np.random.default_rng(9), 8)
    ctx = se.create_context()
    ctx.set_topk(10)
    assert se.search(q, 8, ctx, 16) == 0
    scanned, hops, _ = se.last_stats(ctx, 8)
    for i in range(8):
        r = H.search_model(g, q[i], 10, 16, metric=fx.metric)
        assert ctx.counts[i] == r.keys.size and np.array_equal(ctx.keys[i, :r.keys.size], r.keys)
        assert np.array_equal(ctx.scores[i, :r.keys.size], r.scores) and (scanned[i], hops[i]) == (r.scanned, r.hops)


@pytest.mark.parametrize("name", ["l2-div16-max64", "ip-div1-max64"])
def test_search_on_the_built_graph_equals_the_model(name):
    fx, g, c, _ = B.model_of(name)
    se = _build(fx)
    g = g._replace(keys=_keys(g.rows.shape[0]))
    q = H.exact_queries(g, np.random.default_rng(9), 20)
    ctx = se.create_context()
    for ef, topk in ((32, 10), (5, 5)):
        ctx.set_topk(topk)
        assert se.search(q, 20, ctx, ef) == 0
        scanned, hops, _ = se.last_stats(ctx, 20)
        for i in range(20):
            r = H.search_model(g, q[i], topk, ef, metric=fx.metric)
            assert ctx.counts[i] == r.keys.size and np.array_equal(ctx.keys[i, :r.keys.size], r.keys)
            assert np.array_equal(ctx.scores[i, :r.keys.size], r.scores) and (scanned[i], hops[i]) == (r.scanned, r.hops)


def test_quality_on_gaussian_rows():
    """default rounds; recall@10 at ef 32 is no more than two standard errors below the sequential model's (B.QUALITY_P)"""
    import zvec_amd as zv
    rows, q, levels = B.quality_data()
    p = B.QUALITY_PARAMS
    se = zv.HipHnswSearcher(B.QUALITY_DIM)
    assert se.build(rows, levels=levels, m=p.m, m0=p.m0, ef_construction=p.ef_construction) == 0
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    i = se.info()
    n = B.QUALITY_N
    assert (cnt0 <= p.m0).all() and (cnt_up <= p.m).all()
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
    H.check_graph(H.Graph(rows, keys, p.m0, nbr0, cnt0, i["max_level"], p.m, i["n_upper"], upper_of, nbr_up, cnt_up, i["entry_point"]))
    ctx = se.create_context()
    ctx.set_topk(B.QUALITY_K)
    assert se.search(q, B.QUALITY_Q, ctx, B.QUALITY_EF) == 0
    got = B.recall(ctx.keys, B.quality_truth(rows, q))
    print("recall@10 %.4f, floor %.4f (p = %.4f)" % (got, B.quality_floor(), B.QUALITY_P))
    assert got >= B.quality_floor()


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_build")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "hnsw_build.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_build ok" in out.stdout.decode()

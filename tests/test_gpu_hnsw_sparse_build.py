"""Building an HNSW graph over sparse rows on the GPU (zvec_hip_hnsw_sparse_build*), against hnsw_build_ref.build_model on the rows
densified over their vocabulary, as tests/test_gpu_hnsw_sparse.py densifies them.  Values are the non-zero integers of [-8, 8]: every
sum is an exact fp32 (and the values exact halves), so the exported arrays, info, get_vector and the four counters equal the model's.
On Gaussian values an fp16 handle and an fp32 handle given the widened values must agree bit for bit, and the graph must be valid."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402
from test_gpu_hnsw_build import _keys, _options  # noqa: E402
from test_gpu_hnsw_sparse import ROW_LENS, _dense, _runs  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID = -12, -31
BASE = B.params(m=4, m0=8, ef_construction=16)
# name -> row lengths, rows, vocabulary, parameters, (round_div, round_max)
CASES = {"short": (ROW_LENS["short"], 600, 48, BASE, (16, 64)), "mixed": (ROW_LENS["mixed"], 600, 192, BASE, (16, 64)),
         "long": ([0, 700, 1500, 4096], 120, 4096, BASE, (16, 64)),
         "wide": (ROW_LENS["mixed"], 300, 192, B.params(m=40, m0=80, ef_construction=100), (16, 64)),
         "prune_cnt": (ROW_LENS["mixed"], 300, 192, B.params(m=4, m0=8, ef_construction=16, prune_cnt=2), (16, 64)),
         "min_neighbors": (ROW_LENS["mixed"], 300, 192, B.params(m=4, m0=8, ef_construction=16, min_neighbors=4), (16, 64)),
         "all_whole": (ROW_LENS["mixed"], 300, 192, B.params(m=8, m0=16, ef_construction=6), (16, 64)),
         "n1": (ROW_LENS["mixed"], 1, 192, BASE, (16, 64)), "n2": (ROW_LENS["mixed"], 2, 192, BASE, (16, 64))}


@functools.lru_cache(maxsize=None)
def _model(name, rounds=None, real=False):
    """(fixture, model graph, model counters) of a case, under its own (round_div, round_max) or the given one"""
    lens, n, vocab, p, rd = CASES[name]
    rng = np.random.default_rng([11, n, vocab])
    rows = _dense(rng, rng.choice(lens, n), vocab, real)
    if real:
        rows = rows.astype(np.float16).astype(np.float32)
    fx = B.Fixture(rows, p, B.mid_levels(max(n, 120), p.scaling_factor)[:n], *(rounds or rd), "ip")
    return (fx,) + B.build_model(rows, p, fx.levels, fx.round_div, fx.round_max, "ip", keys=_keys(n))


def _build(fx, dtype="fp32", dev=False, ws_bytes=1 << 30):
    import zvec_amd as zv
    se = zv.HipHnswSparseSearcher(dtype=dtype)
    p = fx.params
    kw = dict(keys=_keys(fx.rows.shape[0]), levels=fx.levels, m=p.m, m0=p.m0, ef_construction=p.ef_construction, prune_cnt=p.prune_cnt,
              min_neighbors=p.min_neighbors)
    c, i, v = _runs(fx.rows)
    with _options(hnsw_build_round_div=fx.round_div, hnsw_build_round_max=fx.round_max, hnsw_ws_bytes=ws_bytes):
        if dev:
            import torch
            di, dv = (torch.from_numpy(x).to(torch.device("cuda:0")) for x in (i.view(np.int32), v.astype(se.np_dtype)))
            torch.cuda.synchronize()
            assert se.build_dev(c, di.data_ptr(), dv.data_ptr(), **kw) == 0
        else:
            assert se.build(c, i, v, **kw) == 0
    return se


def _counters(se):
    b = se.build_info()
    return b["rounds"], b["dists"], b["requests"], b["prunes"]


def _same(se, g, c, what=""):
    """the handle holds the model's graph and rows, array for array, and the build counted what the model counted"""
    i, n = se.info(), g.rows.shape[0]
    assert (i["n"], i["elements"], i["m0"], i["max_level"], i["entry_point"]) == (n, (g.rows != 0).sum(), g.m0, g.max_level, g.entry_point), what
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
    assert np.array_equal(keys, g.keys) and np.array_equal(cnt0, g.cnt0) and np.array_equal(nbr0, g.nbr0), what
    if g.max_level > 0:
        assert (i["m"], i["n_upper"]) == (g.m, g.n_upper), what
        assert np.array_equal(upper_of, g.upper_of) and np.array_equal(cnt_up, g.cnt_up) and np.array_equal(nbr_up, g.nbr_up), what
    else:
        assert upper_of is None
    for pos in range(n):
        gi, gv = se.get_vector_by_id(pos)
        assert np.array_equal(gi, np.nonzero(g.rows[pos])[0]) and np.array_equal(gv, g.rows[pos][g.rows[pos] != 0]), what
    b = se.build_info()
    print(what, "gpu", _counters(se), "model", tuple(c))
    assert _counters(se) == tuple(c) and (b["top"], b["entry_point"]) == (g.max_level, g.entry_point), what
    return b


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rounds", [(0, 64), (16, 64), (1, 64)])
@pytest.mark.parametrize("name", ["short", "mixed"])
def test_exact_rows_equal_the_model(name, rounds, dtype):
    """row lengths around the 16-lane group and its step of two; one node per round, the default division, and rounds as large as
    the graph, where one target receives more requests in a round than its list holds"""
    fx, g, c = _model(name, rounds)
    assert c.prunes > 1000
    _same(_build(fx, dtype), g, c, "%s %s" % (name, rounds))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["long", "wide", "prune_cnt", "min_neighbors", "all_whole", "n1", "n2"])
def test_shapes_and_parameters(name, dtype):
    """rows of 4096 pairs (both runs at their largest, the fp32 launch above 64 KiB of LDS); lists wider than a wave; prune_cnt
    below m; a fill up to min_neighbors; every W taken whole; one and two rows"""
    fx, g, c = _model(name)
    assert name != "long" or c.prunes > 0
    _same(_build(fx, dtype), g, c, name)


def test_no_rows():
    import zvec_amd as zv
    se = zv.HipHnswSparseSearcher()
    with pytest.raises(Exception):
        se.build_info()                        # NoReady before the first build
    none = np.zeros(0, np.uint32)
    assert se.build(none, none, np.zeros(0, np.float32), m=8) == 0
    assert se.info()["n"] == 0 and _counters(se) == (0, 0, 0, 0)
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search(*_runs(np.ones((2, 8), np.float32)), 2, ctx, 8) == 0 and (ctx.counts == 0).all()


def test_slices_and_device_rows():
    fx, g, c = _model("mixed", (1, 64))
    assert B.slices_of(fx, 1024) > 1
    assert _same(_build(fx, ws_bytes=1024), g, c, "sliced")["slices"] == B.slices_of(fx, 1024)
    assert _same(_build(fx, "fp16", dev=True), g, c, "build_dev")["slices"] == 1


def test_search_on_the_built_graph_equals_the_model():
    fx, g, c = _model("mixed")
    se = _build(fx)
    q = _dense(np.random.default_rng(9), [0, 1, 5, 17, 64] * 4, 192)
    ctx = se.create_context()
    for ef, topk in ((32, 10), (5, 5)):
        ctx.set_topk(topk)
        assert se.search(*_runs(q), 20, ctx, ef) == 0
        scanned, hops, _ = se.last_stats(ctx, 20)
        for i in range(20):
            r = H.search_model(g, q[i], topk, ef, metric="ip")
            assert ctx.counts[i] == r.keys.size and np.array_equal(ctx.keys[i, :r.keys.size], r.keys)
            assert np.array_equal(ctx.scores[i, :r.keys.size], r.scores) and (scanned[i], hops[i]) == (r.scanned, r.hops)


def test_real_values_fp16_equals_fp32_and_the_graph_is_valid():
    """Gaussian values rounded to binary16: the two value types build the same graph with the same counters; no recall is asserted"""
    fx = _model("mixed", None, True)[0]
    a, b = _build(fx, "fp16"), _build(fx, "fp32")
    ea, eb = a.export(), b.export()
    assert all(np.array_equal(x, y) for x, y in zip(ea, eb)) and _counters(a) == _counters(b) and a.info() == b.info()
    keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = ea
    i = a.info()
    H.check_graph(H.Graph(fx.rows, keys, i["m0"], nbr0, cnt0, i["max_level"], i["m"], i["n_upper"], upper_of, nbr_up, cnt_up, i["entry_point"]))
    lists = [(v, nbr0[v, :cnt0[v]]) for v in range(600)]
    lists += [(v, nbr_up[upper_of[v], l, :cnt_up[upper_of[v], l]]) for v in np.nonzero(fx.levels)[0] for l in range(i["max_level"])]
    assert all(v not in x and len(set(x.tolist())) == x.size for v, x in lists)


def test_refusals_leave_the_handle_alone():
    fx, g, c = _model("prune_cnt")
    se = _build(fx)
    before = (se.info(), se.build_info())
    cnt, idx, val = _runs(fx.rows)
    kw = dict(levels=fx.levels, m=4, m0=8, ef_construction=16)
    long_c = np.ones(300, np.uint32)
    long_c[7] = 4097
    assert se.build(long_c, np.concatenate([np.arange(x, dtype=np.uint32) for x in long_c]), np.ones(long_c.sum(), np.float32), **kw) == INVALID
    at = int(cnt[:np.nonzero(cnt >= 2)[0][0]].sum())
    swapped = idx.copy()
    swapped[[at, at + 1]] = swapped[[at + 1, at]]
    assert se.build(cnt, swapped, val, **kw) == INVALID
    assert se.build(cnt, idx, val, **dict(kw, min_neighbors=5)) == INVALID
    assert se.build(cnt, idx, val, **dict(kw, ef_construction=513)) == UNSUPPORTED
    assert (se.info(), se.build_info()) == before
    _same(se, g, c, "after the refused builds")


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_sparse_build")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "hnsw_sparse_build.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_sparse_build ok" in out.stdout.decode()

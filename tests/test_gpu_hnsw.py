"""Search on a built HNSW graph on the GPU (zvec_hip_hnsw_*), against the model of tests/hnsw_ref.py.  On exact data (integer rows:
every fp32 distance is exact in any summation order, ties are plentiful) keys, scores, counts, distances computed and nodes expanded
equal the model's bit for bit; on Gaussian rows the queries whose computed distances are all more than two accumulation bands apart
do so too, and every returned score is within one band of the fp64 score of its key."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, MISMATCH, INVALID = -12, -24, -31
NAMES = {"l2": "SquaredEuclidean", "ip": "InnerProduct"}
NOKEY = 0xffffffffffffffff


def _loaded(g, metric="l2"):
    import zvec_amd as zv
    se = zv.HipHnswSearcher(g.rows.shape[1], NAMES[metric])
    up = g.max_level > 0
    assert se.load(g.rows, g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of if up else None, g.nbr_up if up else None,
                   g.cnt_up if up else None) == 0
    return se


def _search(se, q, topk, ef, max_scan=0, threshold=None, exclude=None, ctx=None):
    ctx = ctx or se.create_context()
    ctx.set_topk(topk)
    if threshold is not None:
        ctx.set_threshold(threshold)
    ctx.set_exclude_bitset(None if exclude is None else H.words_of(exclude))
    assert se.search(q, q.shape[0], ctx, ef, max_scan) == 0
    scanned, hops, slices = se.last_stats(ctx, q.shape[0])
    return ctx.keys, ctx.scores, ctx.counts, scanned, hops, slices


def _check(se, g, q, topk, ef, metric="l2", max_scan=0, threshold=None, exclude=None, what="", only=None):
    """one batch against the model: lists, counts and both statistics, bit for bit; only: the queries compared"""
    keys, scores, counts, scanned, hops, _ = _search(se, q, topk, ef, max_scan, threshold, exclude)
    models = []
    for i in (range(q.shape[0]) if only is None else only):
        r = H.search_model(g, q[i], topk, ef, max_scan, threshold, exclude, metric)
        w = "%s query %d" % (what, i)
        assert counts[i] == r.keys.size, w
        assert np.array_equal(keys[i, :counts[i]], r.keys), w
        if only is None:
            assert np.array_equal(scores[i, :counts[i]], r.scores), w
        assert (keys[i, counts[i]:] == NOKEY).all() and np.isinf(scores[i, counts[i]:]).all(), w
        assert (scanned[i], hops[i]) == (r.scanned, r.hops), w
        models.append(r)
    return keys, scores, counts, models


COMBOS = [(1, 1, 7), (10, 1, 1), (10, 10, 64), (64, 10, 7), (64, 64, 7), (512, 10, 7), (512, 512, 1), (10, 10, 200)]      # ef, topk, batch


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim,m", [(4, 4), (20, 8), (100, 4), (128, 8)])
def test_exact_data_equals_the_model(dim, m, metric):
    """dim below, off and on the 16-byte lane grid and the 16-lane group's 64 floats; every ef / topk / batch of the list"""
    g = H.exact_graph(1500, dim, m)
    se = _loaded(g, metric)
    rng = np.random.default_rng([dim, m])
    for ef, topk, batch in COMBOS:
        _check(se, g, H.exact_queries(g, rng, batch), topk, ef, metric, what="ef=%d topk=%d batch=%d" % (ef, topk, batch))


@pytest.mark.parametrize("name", [k for k in H.HAND_MADE])
def test_hand_made_graphs(name):
    g = H.HAND_MADE[name]()
    se = _loaded(g)
    q = np.zeros((5, 4), np.float32)
    q[:, 0] = [0, 10, 30, 12, 8]               # (integers, like the rows: every distance is exact and many tie)
    for ef, topk in ((1, 1), (3, 3), (8, 64), (64, 8)):
        _check(se, g, q, topk, ef, what="%s ef=%d topk=%d" % (name, ef, topk))
    _check(se, g, q, 5, 5, max_scan=3, what=name + " max_scan=3")


def test_empty_index():
    import zvec_amd as zv
    se = zv.HipHnswSearcher(8)
    assert se.load(np.zeros((0, 8), np.float32), np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32)) == 0
    assert se.info()["n"] == 0
    keys, scores, counts, scanned, hops, _ = _search(se, np.ones((3, 8), np.float32), 4, 16)
    assert (counts == 0).all() and (keys == NOKEY).all() and np.isinf(scores).all() and (scanned == 0).all() and (hops == 0).all()


def test_query_equal_to_a_row_and_topk_beyond_the_reachable():
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    keys, scores, _, _ = _check(se, g, g.rows[[5, 700, 1499]], 10, 64)
    assert (scores[:, 0] == 0).all() and keys[:, 0].tolist() == [5 * 7 + 3, 700 * 7 + 3, 1499 * 7 + 3]
    two = H.two_components()
    q = np.array([[12.0, 0, 0, 0]], np.float32)
    keys, _, counts, _ = _check(_loaded(two), two, q, 20, 20)
    assert counts[0] == 5


def test_exclude_bitset():
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    rng = np.random.default_rng(3)
    q = H.exact_queries(g, rng, 6)
    ex = np.zeros(1500, bool)
    ex[g.entry_point] = True
    _check(se, g, q, 10, 32, exclude=ex, what="entry point")
    near = np.zeros(1500, bool)                # a whole neighbourhood: walked through, never returned; C grows past ef
    near[[int(k - 3) // 7 for k in H.search_model(g, q[0], 200, 200).keys]] = True
    keys, _, _, models = _check(se, g, q, 10, 10, exclude=near, what="neighbourhood")
    assert models[0].c_peak > 10 and not set(keys[0].tolist()) & set((np.nonzero(near)[0] * 7 + 3).tolist())
    _, _, counts, models = _check(se, g, q, 10, 10, exclude=np.ones(1500, bool), what="everything")
    assert (counts == 0).all() and models[0].scanned >= 1500


def test_candidates_past_the_lds_set():
    """more than 1024 live candidates: the set moves into the context workspace, at once (a star) and with pops after it"""
    star = H.star(1200)
    _check(_loaded(star), star, np.zeros((2, 4), np.float32), 10, 10, exclude=np.ones(1200, bool), what="star")
    big = H.exact_graph(3000, 20, 8)
    q = H.exact_queries(big, np.random.default_rng(4), 3)
    _, _, _, models = _check(_loaded(big), big, q, 10, 10, exclude=np.ones(3000, bool), what="3000 rows")
    assert models[0].c_peak > H.C_LDS
    half = np.arange(3000) % 2 == 0
    _check(_loaded(big, "ip"), big, q, 10, 16, "ip", exclude=half, what="3000 rows, every other one")


def test_threshold_cuts_the_list():
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    q = H.exact_queries(g, np.random.default_rng(5), 5)
    full = H.search_model(g, q[0], 10, 64)
    for t in (float(full.scores[4]), float(full.scores[4]) - 0.5, -1.0):       # on a score (ties stay), between two, below all
        _, _, counts, _ = _check(se, g, q, 10, 64, threshold=t, what="threshold=%g" % t)
    assert (counts == 0).all()


def test_max_scan():
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    q = H.exact_queries(g, np.random.default_rng(2), 8)
    full = H.search_model(g, q[0], 10, 64)
    for ms in (1, 2, 40, full.scanned // 2, full.scanned, 1500, 100000):      # (2: ends inside the upper levels' count)
        _, _, _, models = _check(se, g, q, 10, 64, max_scan=ms, what="max_scan=%d" % ms)
        assert ms > full.scanned // 2 or models[0].on_limit
    # a max_scan small enough that C overflows
    star, ring = H.star(), H.tie_ring()
    _, _, _, models = _check(_loaded(star), star, np.array([[30, 0, 0, 0]], np.float32), 5, 5, max_scan=10)
    assert models[0].evicted > 0
    _, _, _, models = _check(_loaded(ring), ring, np.zeros((1, 4), np.float32), 8, 64, max_scan=3)
    assert models[0].evicted == 1


def test_slices_are_invisible():
    from zvec_amd import _lib
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    q = H.exact_queries(g, np.random.default_rng(6), 200)
    per_query = 4 * ((1500 + 31) // 32) + 8 * 1500                 # visited words + the candidate region (include/zvec_hip.h)
    whole = _search(se, q, 10, 32)
    assert whole[5] == 1
    L = _lib.lib()
    try:
        for slices, rows in ((3, 67), (17, 12)):
            _lib.check(L.zvec_hip_set_option(b"hnsw_ws_bytes", rows * per_query), "set_option")
            got = _search(se, q, 10, 32)
            assert got[5] == slices
            for a, b in zip(whole[:5], got[:5]):
                assert np.array_equal(a, b)
    finally:
        _lib.check(L.zvec_hip_set_option(b"hnsw_ws_bytes", 1 << 30), "set_option")


def test_search_dev_equals_search():
    import torch
    g = H.exact_graph(1500, 100, 4)
    se = _loaded(g, "ip")
    q = H.exact_queries(g, np.random.default_rng(7), 33)
    ex = np.arange(1500) % 3 == 0
    keys, scores, counts, scanned, hops, _ = _search(se, q, 10, 48, exclude=ex)
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    dex = torch.from_numpy(H.words_of(ex).view(np.int64)).to(dev)
    dk = torch.zeros((33, 10), dtype=torch.int64, device=dev)
    ds = torch.zeros((33, 10), dtype=torch.float32, device=dev)
    dc = torch.zeros(33, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = se.create_context()
    assert se.search_dev(dq.data_ptr(), 33, 10, 48, 0, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx, d_exclude=dex.data_ptr()) == 0
    s2, h2, _ = se.last_stats(ctx, 33)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys) and np.array_equal(ds.cpu().numpy(), scores)
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), counts) and np.array_equal(s2, scanned) and np.array_equal(h2, hops)


def test_two_contexts_from_two_threads():
    g = H.exact_graph(1500, 20, 8)
    se = _loaded(g)
    qs = [H.exact_queries(g, np.random.default_rng(s), 40) for s in (8, 9)]
    want = [_search(se, q, 10, 32) for q in qs]
    got = [None, None]

    def run(i):
        ctx = se.create_context()
        for _ in range(5):
            got[i] = _search(se, qs[i], 10, 32, ctx=ctx)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    for w, r in zip(want, got):
        for a, b in zip(w[:5], r[:5]):
            assert np.array_equal(a, b)


def test_load_twice_and_export():
    a, b = H.tie_ring(), H.bare_upper()
    se = _loaded(a)
    for g in (a, b, a):
        up = g.max_level > 0
        assert se.load(g.rows, g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of, g.nbr_up, g.cnt_up) == 0
        i = se.info()
        assert (i["n"], i["dim"], i["m0"], i["max_level"], i["m"], i["n_upper"], i["entry_point"]) == \
               (g.rows.shape[0], 4, g.m0, g.max_level, g.m, g.n_upper, g.entry_point) and up
        keys, nbr0, cnt0, upper_of, nbr_up, cnt_up = se.export()
        for x, y in ((keys, g.keys), (nbr0, g.nbr0), (cnt0, g.cnt0), (upper_of, g.upper_of), (nbr_up, g.nbr_up), (cnt_up, g.cnt_up)):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert np.array_equal(se.get_vectors_by_ids(np.arange(g.rows.shape[0])), g.rows)
        q = g.rows[:3] + 1
        _check(se, g, q, 5, 16)


def test_refusals():
    from zvec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.zvec_hip_hnsw_create(16, _lib.DT_FP16, _lib.METRIC_L2, 0, C.byref(h)) == UNSUPPORTED
    assert L.zvec_hip_hnsw_create(16, _lib.DT_FP32, _lib.METRIC_COSINE, 0, C.byref(h)) == UNSUPPORTED
    assert L.zvec_hip_hnsw_create(16, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(h)) == UNSUPPORTED
    g = H.bare_upper()
    se = _loaded(g)
    q = np.zeros((2, 4), np.float32)
    before = _search(se, q, 3, 8)

    def load(**kw):
        d = g._asdict()
        d.update(kw)
        return se.load(d["rows"], d["nbr0"], d["cnt0"], d["entry_point"], d["keys"], d["upper_of"], d["nbr_up"], d["cnt_up"])

    bad = g.nbr0.copy(); bad[3, 0] = 12                                    # noqa: E702
    assert load(nbr0=bad) == INVALID
    bad = g.cnt0.copy(); bad[3] = g.m0 + 1                                 # noqa: E702
    assert load(cnt0=bad) == INVALID
    bad = g.nbr_up.copy(); bad[0, 0, 0] = 12                               # noqa: E702
    assert load(nbr_up=bad) == INVALID
    bad = g.nbr_up.copy(); bad[0, 0, 0] = 5                                # (node 5 has no upper lists)   # noqa: E702
    assert load(nbr_up=bad) == INVALID
    bad = g.cnt_up.copy(); bad[1, 0] = g.m + 1                             # noqa: E702
    assert load(cnt_up=bad) == INVALID
    assert load(entry_point=12) == INVALID
    assert load(entry_point=5) == INVALID                                  # (no upper lists while max_level >= 1)
    assert load(rows=np.zeros((12, 5), np.float32)) == MISMATCH
    after = _search(se, q, 3, 8)                                           # the handle was not touched
    for a, b in zip(before[:5], after[:5]):
        assert np.array_equal(a, b)
    ctx = se.create_context()
    ctx.set_topk(3)
    assert se.search(q, 2, ctx, 513) == UNSUPPORTED
    assert se.search(q, 2, ctx, 512) == 0
    ctx.set_topk(513)
    assert se.search(q, 2, ctx, 8) == UNSUPPORTED
    ctx.set_topk(3)
    assert se.search(np.zeros((2, 5), np.float32), 2, ctx, 8) == MISMATCH


@pytest.mark.parametrize("dim", sorted(H.REAL))
def test_real_data(dim):
    g, q = H.real_graph(dim)
    se = _loaded(g)
    models = [H.search_model(g, x, H.REAL_TOPK, H.REAL_EF) for x in q]
    good = [i for i in range(len(q)) if H.decisive(models[i], H.band(g, q[i], models[i].nodes))]
    assert len(good) * 4 >= 3 * len(q)
    _check(se, g, q, H.REAL_TOPK, H.REAL_EF, only=good, what="dim=%d" % dim)
    ex = np.arange(H.REAL_N) % 5 == 0
    pos_of = {int(k): i for i, k in enumerate(g.keys)}
    for ef, topk, exclude in ((H.REAL_EF, H.REAL_TOPK, None), (64, 10, None), (64, 10, ex)):
        keys, scores, counts, _, _, _ = _search(se, q, topk, ef, exclude=exclude)
        for i in range(len(q)):
            b = H.band(g, q[i], H.search_model(g, q[i], topk, ef, exclude=exclude).nodes)
            c = int(counts[i])
            assert c == topk
            pos = [pos_of[int(k)] for k in keys[i, :c]]
            assert len(set(pos)) == c and (exclude is None or not exclude[pos].any())
            assert (np.diff(scores[i, :c]) >= 0).all()
            assert np.abs(scores[i, :c].astype(np.float64) - H.scores64(g.rows[pos], q[i], "l2")).max() <= b


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_search")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "examples", "hnsw_search.c"),
                               "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip", "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_search ok" in out.stdout.decode()

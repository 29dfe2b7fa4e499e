"""HNSW over binary rows under the Hamming distance on the GPU (zvec_hip_hnsw_create_binary, DESIGN §3c "Binary rows").  The Hamming
distance of two bit rows is the squared L2 distance of the rows unpacked to 0/1, an exact fp32 integer, so up to 4096 bits the binary
handle answers bit for bit as W, the fp32 SquaredEuclidean handle given the unpacked rows, and at any width the fp64 models of
hnsw_ref / hnsw_build_ref / hnsw_add_ref / hnsw_group_ref apply as they stand with metric "l2".  No tolerance anywhere.  The helpers
that compare two handles are those of test_gpu_hnsw_f16 and test_gpu_hnsw_group."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_add_ref as A  # noqa: E402
import hnsw_build_ref as B  # noqa: E402
import hnsw_group_ref as G  # noqa: E402
import hnsw_ref as H  # noqa: E402
import test_gpu_hnsw_f16 as F  # noqa: E402
import test_gpu_hnsw_group as TG  # noqa: E402

pytestmark = pytest.mark.gpu

P = B.params(m=8, m0=16, ef_construction=32)
WIDTHS = (32, 96, 128, 160, 768, 2048, 2080, 4096)          # every lane split and its edges; 4096: the last width W exists for
BEYOND = (4128, 32768)                                      # a third step of sixteen lanes; the cap


def _words(n, nbits, seed):
    """uniform random bit rows; exact duplicates, an all-zero and an all-ones row planted"""
    w = np.random.default_rng([seed, nbits]).integers(0, 1 << 32, (n, nbits // 32), dtype=np.uint64).astype(np.uint32)
    if n >= 8:
        w[3], w[n - 1], w[4], w[5] = w[1], w[1], 0, 0xffffffff
    return w


def _unpack(w):
    return np.unpackbits(np.ascontiguousarray(w).view(np.uint8), axis=1, bitorder="little").astype(np.float32)


def _searcher(nbits, dtype="binary32"):
    import zvec_amd as zv
    return zv.HipHnswSearcher(nbits, "SquaredEuclidean" if dtype == "fp32" else "Hamming", dtype=dtype)


def _give(se, w):
    """bit rows as this handle takes them: words of its type, or 0/1 floats for W"""
    return _unpack(w) if se.np_dtype is np.float32 else np.ascontiguousarray(w).view(se.np_dtype)


def _graphs(nbits, n=200):
    """(graph over the unpacked rows, the rows as words): one from hnsw_ref.build_graph with lists of at most 10, three hand-made"""
    w = _words(n, nbits, 1)
    yield H.build_graph(_unpack(w), 5, 24, 7), w
    for name in ("star", "single", "with_empty_lists"):
        g = H.HAND_MADE[name]()
        w = _words(g.rows.shape[0], nbits, 2)
        yield g._replace(rows=_unpack(w)), w


def _loaded(g, w, dtype="binary32"):
    se = _searcher(w.shape[1] * 32, dtype)
    up = [g.upper_of, g.nbr_up, g.cnt_up] if g.max_level > 0 else [None] * 3
    assert se.load(_give(se, w), g.nbr0, g.cnt0, g.entry_point, g.keys, *up) == 0
    return se


def _search(se, qw, topk, ef, max_scan=0, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(topk)
    if threshold is not None:
        ctx.set_threshold(threshold)
    ctx.set_exclude_bitset(None if exclude is None else H.words_of(exclude))
    assert se.search(_give(se, qw), qw.shape[0], ctx, ef, max_scan) == 0
    return (ctx.keys, ctx.scores, ctx.counts) + tuple(se.last_stats(ctx, qw.shape[0]))


def _equals_model(res, g, qw, topk, ef, what, **kw):
    keys, scores, counts, scanned, hops, _ = res
    for i, q in enumerate(_unpack(qw)):
        r = H.search_model(g, q, topk, ef, **kw)
        assert counts[i] == r.keys.size and (scanned[i], hops[i]) == (r.scanned, r.hops), (what, i)
        assert keys[i, :counts[i]].tobytes() == r.keys.tobytes() and scores[i, :counts[i]].tobytes() == r.scores.tobytes(), (what, i)
        assert (keys[i, counts[i]:] == F.NOKEY).all() and np.isinf(scores[i, counts[i]:]).all(), (what, i)


def _same_graph(se, g, w, what=""):
    """the handle holds the model's graph, array for array, and the words that went in; dim is reported in bits"""
    i, n = se.info(), g.rows.shape[0]
    assert (i["n"], i["dim"], i["m0"], i["max_level"], i["entry_point"]) == (n, w.shape[1] * 32, g.m0, g.max_level, g.entry_point), what
    want = [g.keys, g.nbr0, g.cnt0] + ([g.upper_of, g.nbr_up, g.cnt_up] if g.max_level > 0 else [None] * 3)
    for x, y in zip(se.export(), want):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), what
    assert se.get_vectors_by_ids(np.arange(n)).tobytes() == w[:n].tobytes(), what


@pytest.mark.parametrize("nbits", WIDTHS + BEYOND)
def test_search_equals_the_twin_and_the_model(nbits):
    for g, w in _graphs(nbits, 200 if nbits in WIDTHS else 48):
        n = w.shape[0]
        h, t = _loaded(g, w), _loaded(g, w, "fp32") if nbits in WIDTHS else None
        qw = _words(6, nbits, 3)
        qw[1] = w[n // 2]
        thr = float(np.sort(_search(h, qw, 10, 24)[1][:, 0])[3])        # the best score of a middle query: cuts some lists, not all
        for kw in (dict(), dict(exclude=np.arange(n) % 3 == 0), dict(threshold=thr), dict(max_scan=max(2, n // 4))):
            what = "%d bits, n=%d, %s" % (nbits, n, sorted(kw))
            res = _search(h, qw, 10, 24, **kw)
            if t is not None:
                F._same_bits(res, _search(t, qw, 10, 24, **kw), what)
            _equals_model(res, g, qw, 10, 24, what, **kw)
        if nbits == 768:                                                # BINARY64: the same bytes, the same answers
            b = _loaded(g, w, "binary64")
            F._same_bits(_search(h, qw, 10, 24), _search(b, qw, 10, 24), "binary64")
            got = b.get_vectors_by_ids(np.arange(n))
            assert got.dtype == np.uint64 and got.tobytes() == w.tobytes() and b.info()["dim"] == 768


@pytest.mark.parametrize("nbits,dev,div,ws", [(b, d, 16, 1 << 30) for b in (32, 768, 2080) for d in (False, True)] + [(768, False, 4, 1024)])
def test_build_equals_the_twin_and_the_model(nbits, dev, div, ws):
    """host and device rows; the last case: rounds of up to 75 nodes under a workspace for 25 waves, which go in slices"""
    import torch
    n = 300
    w, lv, keys = _words(n, nbits, 4), B.levels_model(n, P.scaling_factor, 5), A._keys(n)
    g, c = B.build_model(_unpack(w), P, lv, div, 4096, "l2", keys=keys)
    slices = B.slices_of(B.Fixture(None, P, lv, div, 4096, "l2"), ws)
    h, t = _searcher(nbits), _searcher(nbits, "fp32")
    for se in (h, t):
        d = torch.from_numpy(_give(se, w).view(np.int32)).cuda()
        torch.cuda.synchronize()
        with F._options(hnsw_build_round_div=div, hnsw_ws_bytes=ws):
            kw = dict(keys=keys, levels=lv, **F._params(P))
            assert (se.build_dev(d.data_ptr(), n, **kw) if dev else se.build(_give(se, w), **kw)) == 0
    assert F._pick(h.build_info(), F.COUNTERS) == F._pick(t.build_info(), F.COUNTERS) and (slices > 1) == (ws == 1024)
    assert F._pick(h.build_info(), ("slices", "rounds", "dists", "requests", "prunes")) == (slices,) + tuple(c) and c.prunes > 0
    F._export_equal(h, t, "build")
    _same_graph(h, g, w, "build")


def test_add_in_two_calls_equals_the_twin_and_the_model():
    """an add that builds (200 rows), then adds of 40 and of 20 rows; a row of the last call raises the top level"""
    n = 260
    w, keys = _words(n, 768, 6), A._keys(n)
    lv = np.minimum(B.levels_model(n, P.scaling_factor, 5), 1)
    lv[250] = 3
    calls = A.add_model(_unpack(w), P, lv, (200, 40, 20), keys=keys)
    assert calls[2].restrided and not calls[1].restrided
    h, t = _searcher(768), _searcher(768, "fp32")
    for k in calls:
        a, e = k.first, k.first + k.count
        for se in (h, t):
            assert se.add(_give(se, w[a:e]), keys=keys[a:e], levels=lv[a:e], **F._params(P)) == 0
        i = h.add_info()
        assert F._pick(i, F.ADD_COUNTERS) == F._pick(t.add_info(), F.ADD_COUNTERS), a
        assert F._pick(i, ("rounds", "dists", "requests", "prunes", "restrided")) == tuple(k.counters) + (k.restrided,), a
        F._export_equal(h, t, "call at %d" % a)
        _same_graph(h, k.graph, w, "call at %d" % a)


@pytest.mark.parametrize("gnum,gk,expands", [(2, 3, False), (6, 1, True)])
def test_group_by_equals_the_twin_and_the_model(gnum, gk, expands):
    """seven groups and a result list of six: two groups are always among them, six only when G3 has walked on"""
    g, w = next(_graphs(768))
    qw = _words(6, 768, 3)
    c = G._case(g, _unpack(qw), np.arange(w.shape[0]) % 7, gnum, gk, 4, None)
    ms = G.model_of(c)
    assert all(m.expanded for m in ms) if expands else not any(m.expanded for m in ms)
    a, b = TG._search(_loaded(g, w), c._replace(q=qw)), TG._search(_loaded(g, w, "fp32"), c)
    assert [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]
    TG._equals_model(a, ms, c)


def test_plumbing_and_refusals():
    import zvec_amd as zv
    from zvec_amd import _lib
    L, out, d = _lib.lib(), C.c_void_p(0x55), C.c_int(-1)
    B32, B64 = _lib.DT_BINARY32, _lib.DT_BINARY64
    for nbits, dt, want in ((0, B32, F.INVALID), (48, B32, F.INVALID), (96, B64, F.INVALID), (32800, B32, F.UNSUPPORTED),
                            (64, _lib.DT_FP32, F.UNSUPPORTED), (64, _lib.DT_FP16, F.UNSUPPORTED)):
        assert L.zvec_hip_hnsw_create_binary(nbits, dt, 0, C.byref(out)) == want and out.value == 0x55, (nbits, dt)
    assert L.zvec_hip_hnsw_create_binary(64, B32, 0, None) == F.INVALID
    for create in (L.zvec_hip_hnsw_create, L.zvec_hip_hnsw_create_typed):
        assert create(64, B32, _lib.METRIC_HAMMING, 0, C.byref(out)) == F.UNSUPPORTED and out.value == 0x55
    with pytest.raises(_lib.ZvecHipError):
        zv.HipHnswSearcher(64, dtype="binary32")                       # the default metric: where it went before
    for name, dt, words in (("binary32", B32, np.uint32), ("binary64", B64, np.uint64)):
        se = _searcher(32768, name)
        assert L.zvec_hip_hnsw_dtype(se._h, C.byref(d)) == 0 and d.value == dt and se.np_dtype is words and se.info()["dim"] == 32768
    assert se.load(np.zeros((3, 511), np.uint64), np.zeros((3, 2), np.uint32), np.zeros(3, np.uint32)) == F.MISMATCH


def test_c_example_runs(tmp_path):
    exe = str(tmp_path / "hnsw_hamming")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(F.ROOT, "include"), "-o", exe,
                           os.path.join(F.ROOT, "examples", "hnsw_hamming.c"), "-L" + os.path.join(F.ROOT, "zvec_amd"), "-lzvec_hip",
                           "-Wl,-rpath," + os.path.join(F.ROOT, "zvec_amd")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and "hnsw_hamming ok" in out.stdout.decode(), out.stdout.decode()

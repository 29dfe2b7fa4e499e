"""Search on a built HNSW graph over sparse rows on the GPU (zvec_hip_hnsw_sparse_*), against the model of tests/hnsw_ref.py on the
rows densified over their small vocabulary (there the dense inner product IS the sparse one).  On exact data (integer values: every
fp32 sum is exact in any order) keys, scores, counts, distances computed and nodes expanded equal the model's bit for bit; an fp16
handle equals the fp32 handle given the widened values bit for bit on real values; on Gaussian values the decisive queries equal the
model and every returned score is within one band of fp64."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID = -12, -31
NOKEY = 0xffffffffffffffff
N, VOCAB = 1500, 512
ROW_LENS = {"short": [0, 1, 15, 16, 17], "mixed": [0, 1, 15, 16, 17, 31, 32, 33, 64, 65, 130]}      # around the 16-lane group and its step of two
Q_LENS = [0, 1, 2, 3, 5, 16, 17, 64, 65, 300]          # every halving count's edge, the empty query, a run longer than a wave
COMBOS = [(1, 1, 7), (10, 10, 64), (64, 10, 7), (512, 512, 1)]          # ef, topk, batch
INTS = np.array([v for v in range(-8, 9) if v], np.float32)


def _dense(rng, lens, vocab, real=False):
    """rows of the given lengths over `vocab`, densified: random supports, integer values in [-8, 8] without 0, or Gaussian ones"""
    d = np.zeros((len(lens), vocab), np.float32)
    for i, c in enumerate(lens):
        d[i, rng.choice(vocab, int(c), replace=False)] = rng.standard_normal(int(c)) if real else rng.choice(INTS, int(c))
    return d


def _runs(dense):
    """dense rows -> counts, indices, values with the zeros dropped (row-major, so ascending inside a row)"""
    nz = dense != 0
    return nz.sum(1).astype(np.uint32), np.nonzero(nz)[1].astype(np.uint32), dense[nz]


@functools.lru_cache(maxsize=None)
def _exact(profile, n=N, vocab=VOCAB, m=8):
    rng = np.random.default_rng([7, n, vocab, len(profile)])
    return H.build_graph(_dense(rng, rng.choice(ROW_LENS[profile], n), vocab), m, 24, 5, metric="ip")


def _queries(g, rng, count, off=0):
    return _dense(rng, [Q_LENS[(j + off) % len(Q_LENS)] for j in range(count)], g.rows.shape[1])


def _loaded(g, dtype="fp32"):
    import zvec_amd as zv
    se = zv.HipHnswSparseSearcher(dtype=dtype)
    up = g.max_level > 0
    assert se.load(*_runs(g.rows), g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of if up else None, g.nbr_up if up else None,
                   g.cnt_up if up else None) == 0
    return se


def _search(se, q, topk, ef, max_scan=0, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(topk)
    if threshold is not None:
        ctx.set_threshold(threshold)
    ctx.set_exclude_bitset(None if exclude is None else H.words_of(exclude))
    assert se.search(*_runs(q), q.shape[0], ctx, ef, max_scan) == 0
    scanned, hops, slices = se.last_stats(ctx, q.shape[0])
    return ctx.keys, ctx.scores, ctx.counts, scanned, hops, slices


def _check(se, g, q, topk, ef, max_scan=0, threshold=None, exclude=None, what="", only=None):
    """one batch against the model as tests/test_gpu_hnsw.py::_check: lists, counts, the fill and both statistics, bit for bit"""
    keys, scores, counts, scanned, hops, _ = _search(se, q, topk, ef, max_scan, threshold, exclude)
    models = []
    for i in (range(q.shape[0]) if only is None else only):
        r = H.search_model(g, q[i], topk, ef, max_scan, threshold, exclude, "ip")
        w = "%s query %d" % (what, i)
        assert counts[i] == r.keys.size, w
        assert np.array_equal(keys[i, :counts[i]], r.keys), w
        if only is None:
            assert np.array_equal(scores[i, :counts[i]], r.scores), w
        assert (keys[i, counts[i]:] == NOKEY).all() and np.isinf(scores[i, counts[i]:]).all(), w
        assert (scanned[i], hops[i]) == (r.scanned, r.hops), w
        models.append(r)
    return keys, scores, counts, models


@pytest.mark.parametrize("profile", sorted(ROW_LENS))
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_exact_data_equals_the_model(dtype, profile):
    g = _exact(profile)
    se = _loaded(g, dtype)
    rng = np.random.default_rng(len(profile))
    for off, (ef, topk, batch) in enumerate(COMBOS):
        _check(se, g, _queries(g, rng, batch, 3 * off), topk, ef, what="ef=%d topk=%d batch=%d" % (ef, topk, batch))


@pytest.mark.parametrize("name", [k for k in H.HAND_MADE])
def test_hand_made_graphs(name):
    g = H.HAND_MADE[name]()                    # (node 0 of the line fixtures is an empty row, query 0 an empty run)
    se = _loaded(g)
    q = np.zeros((5, 4), np.float32)
    q[:, 0] = [0, 10, 30, 12, 8]
    q[3, 1] = -2
    for ef, topk in ((1, 1), (3, 3), (8, 64), (64, 8)):
        _check(se, g, q, topk, ef, what="%s ef=%d topk=%d" % (name, ef, topk))
    _check(se, g, q, 5, 5, max_scan=3, what=name + " max_scan=3")


@pytest.mark.parametrize("case", ["entry", "everything", "third", "max_scan", "threshold"])
def test_exclude_max_scan_and_threshold(case):
    n = 2600 if case == "everything" else N   # (the model's C passes 1024 entries only on the larger graph: 0.5 n at its peak)
    g = _exact("mixed", n)
    se = _loaded(g)
    q = _queries(g, np.random.default_rng(3), 6, 4)
    if case == "entry":
        _check(se, g, q, 10, 32, exclude=np.arange(N) == g.entry_point)
    elif case == "everything":                 # nothing fills R, so C holds every node seen and not yet expanded: past the LDS set
        _, _, counts, models = _check(se, g, q, 10, 10, exclude=np.ones(n, bool))
        assert (counts == 0).all() and min(r.c_peak for r in models) > H.C_LDS
    elif case == "third":
        _check(se, g, q, 10, 16, exclude=np.arange(N) % 3 == 0)
    elif case == "max_scan":
        full = H.search_model(g, q[1], 10, 64, metric="ip")
        for ms in (1, 2, 40, full.scanned // 2, N, 100000):
            _, _, _, models = _check(se, g, q, 10, 64, max_scan=ms, what="max_scan=%d" % ms)
            assert ms > full.scanned // 2 or models[1].on_limit
    else:
        full = H.search_model(g, q[2], 10, 64, metric="ip")
        for t in (float(full.scores[4]), float(full.scores[4]) - 0.5, float(full.scores[0]) - 1.0):      # on a score, between two, below all
            _check(se, g, q, 10, 64, threshold=t, what="threshold=%g" % t)


def test_slices_are_invisible():
    from zvec_amd import _lib
    g = _exact("mixed")
    se = _loaded(g)
    q = _queries(g, np.random.default_rng(6), 40)
    per_query = 4 * ((N + 31) // 32) + 8 * N               # visited words + the candidate region (include/zvec_hip.h)
    whole = _search(se, q, 10, 32)
    assert whole[5] == 1
    L = _lib.lib()
    try:
        _lib.check(L.zvec_hip_set_option(b"hnsw_ws_bytes", 12 * per_query), "set_option")
        got = _search(se, q, 10, 32)
        assert got[5] == 4
        for a, b in zip(whole[:5], got[:5]):
            assert np.array_equal(a, b)
    finally:
        _lib.check(L.zvec_hip_set_option(b"hnsw_ws_bytes", 1 << 30), "set_option")


def test_search_dev_equals_search():
    import torch
    g = _exact("mixed")
    se = _loaded(g, "fp16")
    q = _queries(g, np.random.default_rng(7), 33)
    ex = np.arange(N) % 3 == 0
    keys, scores, counts, scanned, hops, _ = _search(se, q, 10, 48, exclude=ex)
    dev = torch.device("cuda:0")
    c, i, v = _runs(q)
    di, dv = torch.from_numpy(i.view(np.int32)).to(dev), torch.from_numpy(v.astype(np.float16)).to(dev)
    dex = torch.from_numpy(H.words_of(ex).view(np.int64)).to(dev)
    dk = torch.zeros((33, 10), dtype=torch.int64, device=dev)
    ds = torch.zeros((33, 10), dtype=torch.float32, device=dev)
    dc = torch.zeros(33, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = se.create_context()
    assert se.search_dev(c, di.data_ptr(), dv.data_ptr(), 33, 10, 48, 0, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx,
                         d_exclude=dex.data_ptr()) == 0
    s2, h2, _ = se.last_stats(ctx, 33)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys) and np.array_equal(ds.cpu().numpy(), scores)
    assert np.array_equal(dc.cpu().numpy().view(np.uint32), counts) and np.array_equal(s2, scanned) and np.array_equal(h2, hops)


# seed of the real-data fixture: the model alone shows that at least 3/4 of its queries are decisive (25 of 32)
REAL_SEED, REAL_VOCAB, REAL_LENS = 22, 96, [4, 9, 16, 17, 33]


@functools.lru_cache(maxsize=None)
def _real(half):
    """Gaussian values on random supports (rounded to binary16 when `half`), short walks as hnsw_ref.REAL: m 4, ef 4, topk 4"""
    rng = np.random.default_rng(REAL_SEED)
    rows = _dense(rng, rng.choice(REAL_LENS, H.REAL_N), REAL_VOCAB, real=True)
    q = _dense(rng, rng.choice(REAL_LENS, H.REAL_Q), REAL_VOCAB, real=True)
    if half:
        rows, q = rows.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    return H.build_graph(rows, H.REAL_M, 24, REAL_SEED, metric="ip"), q


def test_fp16_equals_fp32_on_the_widened_values():
    g, q = _real(True)
    a, b = _loaded(g, "fp16"), _loaded(g, "fp32")
    ex = np.arange(H.REAL_N) % 5 == 0
    for ef, topk, exclude, ms in ((4, 4, None, 0), (64, 10, None, 0), (64, 10, ex, 0), (512, 100, None, 300)):
        for x, y in zip(_search(a, q, topk, ef, ms, exclude=exclude), _search(b, q, topk, ef, ms, exclude=exclude)):
            assert np.array_equal(x, y)


def _band(g, q, ids):
    """hnsw_ref.band with the count of the longer of the two runs in place of dim"""
    longest = max(int((q != 0).sum()), int((g.rows[ids] != 0).sum(1).max()))
    return H.band(g, q, ids) * (longest + 8) / (g.rows.shape[1] + 8)


def test_real_data():
    g, q = _real(False)
    se = _loaded(g)
    models = [H.search_model(g, x, H.REAL_TOPK, H.REAL_EF, metric="ip") for x in q]
    good = [i for i in range(len(q)) if H.decisive(models[i], _band(g, q[i], models[i].nodes))]
    assert len(good) * 4 >= 3 * len(q)
    keys, scores, counts, _ = _check(se, g, q, H.REAL_TOPK, H.REAL_EF, only=good)
    pos_of = {int(k): i for i, k in enumerate(g.keys)}
    for i in range(len(q)):
        pos = [pos_of[int(k)] for k in keys[i, :counts[i]]]
        assert counts[i] == H.REAL_TOPK and len(set(pos)) == H.REAL_TOPK and (np.diff(scores[i]) >= 0).all()
        assert np.abs(scores[i].astype(np.float64) - H.scores64(g.rows[pos], q[i], "ip")).max() <= _band(g, q[i], models[i].nodes)


def test_longest_query_and_refusals():
    from zvec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    for dtype, metric in ((_lib.DT_BINARY32, _lib.METRIC_IP), (_lib.DT_FP32, _lib.METRIC_L2), (_lib.DT_FP32, _lib.METRIC_COSINE)):
        assert L.zvec_hip_hnsw_sparse_create(dtype, metric, 0, C.byref(h)) == UNSUPPORTED and not h.value
    vocab = 4300
    rng = np.random.default_rng(9)
    g = H.build_graph(_dense(rng, rng.choice(ROW_LENS["mixed"], 200), vocab), 4, 24, 9, metric="ip")
    se = _loaded(g)
    q = _dense(rng, [4096, 3, 4095], vocab)
    before = _check(se, g, q, 5, 16)[:3]

    def load(counts=None, indices=None, **kw):
        c, i, v = _runs(g.rows)
        d = g._asdict()
        d.update(kw)
        if counts is not None:
            c, i, v = counts, indices, np.ones(indices.size, np.float32)
        return se.load(c, i, v, d["nbr0"], d["cnt0"], d["entry_point"], d["keys"], d["upper_of"], d["nbr_up"], d["cnt_up"])

    c, i, _ = _runs(g.rows)
    long_c = np.full(200, 1, np.uint32)
    long_c[7] = 4097
    assert load(long_c, np.concatenate([np.arange(x, dtype=np.uint32) for x in long_c])) == INVALID
    first = int(np.nonzero(c >= 2)[0][0])
    swapped = i.copy()
    at = int(c[:first].sum())
    swapped[[at, at + 1]] = swapped[[at + 1, at]]
    assert load(c, swapped) == INVALID
    bad = g.nbr0.copy(); bad[3, 0] = 200                                   # noqa: E702
    assert load(nbr0=bad) == INVALID
    ctx = se.create_context()
    ctx.set_topk(5)
    assert se.search(*_runs(q), 3, ctx, 513) == UNSUPPORTED
    qc, qi, qv = _runs(q[:2])
    assert se.search(np.array([4097, 3], np.uint32), np.arange(4100, dtype=np.uint32), np.ones(4100, np.float32), 2, ctx, 8) == INVALID
    assert se.search(qc, qi[::-1].copy(), qv, 2, ctx, 8) == INVALID
    for x, y in zip(before, _check(se, g, q, 5, 16)[:3]):                  # the handle was not touched
        assert np.array_equal(x, y)


def test_empty_index_and_read_back():
    import zvec_amd as zv
    se = zv.HipHnswSparseSearcher(dtype="fp16")
    none = np.zeros(0, np.uint32)
    assert se.load(none, none, np.zeros(0, np.float16), np.zeros((0, 4), np.uint32), none) == 0
    assert se.info()["n"] == 0
    keys, scores, counts, scanned, hops, _ = _search(se, np.ones((3, 8), np.float32), 4, 16)
    assert (counts == 0).all() and (keys == NOKEY).all() and np.isinf(scores).all() and (scanned == 0).all() and (hops == 0).all()
    g = H.tie_ring()                           # a second load replaces the first; everything reads back as it went in
    c, i, v = _runs(g.rows)
    assert se.load(c, i, v, g.nbr0, g.cnt0, g.entry_point, g.keys, g.upper_of, g.nbr_up, g.cnt_up) == 0
    info = se.info()
    assert (info["n"], info["elements"], info["m0"], info["max_level"], info["n_upper"]) == (64, i.size, g.m0, g.max_level, g.n_upper)
    for x, y in zip(se.export(), (g.keys, g.nbr0, g.cnt0, g.upper_of, g.nbr_up, g.cnt_up)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    gi, gv = se.get_vector_by_id(5)
    assert gv.dtype == np.float16 and np.array_equal(gi, np.nonzero(g.rows[5])[0]) and np.array_equal(gv, g.rows[5][g.rows[5] != 0])
    assert se.get_vector_by_id(0)[0].size == 0 and se.get_vector_by_id(64) is None
    _check(se, g, g.rows[:3] + 1, 5, 16)


def test_c_example_runs():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "hnsw_sparse_search")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "examples", "hnsw_sparse_search.c"), "-L" + os.path.join(ROOT, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "zvec_amd")])
        out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
        assert out.returncode == 0, out.stdout.decode()
        assert "hnsw_sparse_search ok" in out.stdout.decode()

"""HNSW over int8 rows on the GPU (zvec_hip_hnsw_create_typed(ZVEC_HIP_DT_INT8), DESIGN §3c "int8 rows") and the fp32 -> int8
quantiser.  A score is an exact integer sum converted to fp32.  While every partial sum is an integer below 2^24 (-128 .. 127 at
dim <= 256: 256 * 255^2 < 2^24; |v| <= 31 at dim <= 4096: 4096 * 62^2 < 2^24) fp32 is exact in any order, so the int8 handle answers
bit for bit as W, the fp32 handle given the widened values, and as the fp64 models on the widened rows.  Beyond that range the scores
are checked against exact int64 sums.  No tolerance anywhere; the helpers are those of test_gpu_hnsw_f16 and test_gpu_hnsw_group."""
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
# (dim, largest |v|): 1, 4, 8 and 16 lanes a row; 772: the sixteen-lane stride and a last chunk that is part padding; 4096: the cap
SHAPES = ((4, 128), (60, 128), (128, 128), (256, 128), (772, 31), (4096, 31))


def _rows(n, dim, amp, seed):
    """int8 rows in the twin's range: -128 .. 127, or -31 .. 31; duplicates, a zero row and both extremes planted"""
    top = min(amp, 127)
    assert dim * (amp + top) ** 2 < 1 << 24                         # every partial sum of W is an exact fp32 integer
    r = np.random.default_rng([seed, dim]).integers(-amp, top + 1, (n, dim)).astype(np.int8)
    if n >= 8:
        r[3], r[n - 1], r[4], r[5], r[6] = r[1], r[1], 0, -amp, top
    return r


def _searcher(dim, metric, dtype="int8"):
    import zvec_amd as zv
    return zv.HipHnswSearcher(dim, F.NAMES[metric], dtype=dtype)


def _give(se, r):
    return np.ascontiguousarray(r, se.np_dtype)                     # the bytes, or the widened values for W


def _loaded(g, r, metric, dtype="int8"):
    se = _searcher(r.shape[1], metric, dtype)
    up = [g.upper_of, g.nbr_up, g.cnt_up] if g.max_level > 0 else [None] * 3
    assert se.load(_give(se, r), g.nbr0, g.cnt0, g.entry_point, g.keys, *up) == 0
    return se


def _search(se, q, topk, ef, max_scan=0, threshold=None, exclude=None):
    ctx = se.create_context()
    ctx.set_topk(topk)
    if threshold is not None:
        ctx.set_threshold(threshold)
    ctx.set_exclude_bitset(None if exclude is None else H.words_of(exclude))
    assert se.search(_give(se, q), q.shape[0], ctx, ef, max_scan) == 0
    return (ctx.keys, ctx.scores, ctx.counts) + tuple(se.last_stats(ctx, q.shape[0]))


def _same_graph(se, g, r, what):
    """the handle holds the model's graph, array for array, and the bytes that went in; dim is reported in elements"""
    i, n = se.info(), g.rows.shape[0]
    assert (i["n"], i["dim"], i["m0"], i["max_level"], i["entry_point"]) == (n, r.shape[1], g.m0, g.max_level, g.entry_point), what
    want = [g.keys, g.nbr0, g.cnt0] + ([g.upper_of, g.nbr_up, g.cnt_up] if g.max_level > 0 else [None] * 3)
    for x, y in zip(se.export(), want):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), what
    got = se.get_vectors_by_ids(np.arange(n))
    assert got.dtype == np.int8 and got.tobytes() == r[:n].tobytes(), what


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dim,amp", SHAPES)
def test_search_equals_the_twin_and_the_model(dim, amp, metric):
    n = 200
    r, q = _rows(n, dim, amp, 1), _rows(6, dim, amp, 3)
    q[1] = r[n // 2]
    g = H.build_graph(r.astype(np.float32), 5, 24, 7, metric)
    h, t = _loaded(g, r, metric), _loaded(g, r, metric, "fp32")
    thr = float(np.sort(_search(h, q, 10, 24)[1][:, 0])[3])         # the best score of a middle query: cuts some lists, not all
    for kw in (dict(), dict(exclude=np.arange(n) % 3 == 0, threshold=thr, max_scan=n // 4)):
        res = _search(h, q, 10, 24, **kw)
        F._same_bits(res, _search(t, q, 10, 24, **kw), str(sorted(kw)))
        for i in range(q.shape[0]):
            m = H.search_model(g, q[i].astype(np.float32), 10, 24, metric=metric, **kw)
            assert res[2][i] == m.keys.size and (res[3][i], res[4][i]) == (m.scanned, m.hops), (sorted(kw), i)
            assert res[0][i, :m.keys.size].tobytes() == m.keys.tobytes() and res[1][i, :m.keys.size].tobytes() == m.scores.tobytes(), i


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_sums_beyond_fp32_integers_convert_once(metric):
    """dim 4096 over the full range, -128 against -128 and against 127 among them: sums up to 4096 * 255^2, far above 2^24.  On a
    complete level-0 graph at ef = n every node is scored; each score is np.float32(the exact int64 sum), the order (score, node)"""
    n, dim = 64, 4096
    rng = np.random.default_rng(9)
    r, q3 = rng.integers(-128, 128, (n, dim)).astype(np.int8), rng.integers(-128, 128, dim).astype(np.int8)
    r[0], r[1], r[2, ::2] = -128, 127, -128
    r[8:24] = np.clip(q3.astype(np.int64) + rng.integers(-9, 10, (16, dim)), -128, 127)          # large dot products with q3
    q = np.stack([r[0], r[1], r[7], q3])
    g = H.graph_of(r, [[j for j in range(n) if j != i] for i in range(n)], entry_point=5)
    keys, scores, counts = _search(_loaded(g, r, metric), q, n, n)[:3]
    r64, q64 = r.astype(np.int64), q.astype(np.int64)
    exact = -(q64 @ r64.T) if metric == "ip" else ((r64[None] - q64[:, None]) ** 2).sum(2)
    want = exact.astype(np.float32)
    assert (want.astype(np.int64) != exact).sum() >= 8                                          # (conversions that round)
    for i in range(q.shape[0]):
        order = np.lexsort((np.arange(n), want[i]))
        assert counts[i] == n and keys[i].tolist() == order.tolist() and scores[i].tobytes() == want[i, order].tobytes(), i


@pytest.mark.parametrize("dim,metric,dev,div", [(60, "l2", False, 0), (60, "ip", True, 16), (128, "ip", False, 16), (128, "l2", True, 0)])
def test_build_equals_the_twin_and_the_model(dim, metric, dev, div):
    import torch
    n = 300
    r, lv, keys = _rows(n, dim, 128, 4), B.levels_model(n, P.scaling_factor, 5), A._keys(n)
    g, c = B.build_model(r.astype(np.float32), P, lv, div, 4096, metric, keys=keys)
    h, t = _searcher(dim, metric), _searcher(dim, metric, "fp32")
    for se in (h, t):
        d = torch.from_numpy(_give(se, r)).cuda()
        torch.cuda.synchronize()
        with F._options(hnsw_build_round_div=div):
            kw = dict(keys=keys, levels=lv, **F._params(P))
            assert (se.build_dev(d.data_ptr(), n, **kw) if dev else se.build(_give(se, r), **kw)) == 0
    assert F._pick(h.build_info(), F.COUNTERS) == F._pick(t.build_info(), F.COUNTERS)
    assert F._pick(h.build_info(), ("rounds", "dists", "requests", "prunes")) == tuple(c) and c.prunes > 0
    F._export_equal(h, t, "build")
    _same_graph(h, g, r, "build")


def test_add_in_two_calls_equals_the_twin_and_the_model():
    """an add that builds (200 rows), then adds of 40 and of 20 rows; a row of the last call raises the top level"""
    n, dim = 260, 772
    r, keys = _rows(n, dim, 31, 6), A._keys(n)
    lv = np.minimum(B.levels_model(n, P.scaling_factor, 5), 1)
    lv[250] = 3
    calls = A.add_model(r.astype(np.float32), P, lv, (200, 40, 20), keys=keys)
    assert calls[2].restrided and not calls[1].restrided
    h, t = _searcher(dim, "l2"), _searcher(dim, "l2", "fp32")
    for k in calls:
        a, e = k.first, k.first + k.count
        for se in (h, t):
            assert se.add(_give(se, r[a:e]), keys=keys[a:e], levels=lv[a:e], **F._params(P)) == 0
        i = h.add_info()
        assert F._pick(i, F.ADD_COUNTERS) == F._pick(t.add_info(), F.ADD_COUNTERS), a
        assert F._pick(i, ("rounds", "dists", "requests", "prunes", "restrided")) == tuple(k.counters) + (k.restrided,), a
        F._export_equal(h, t, "call at %d" % a)
        _same_graph(h, k.graph, r, "call at %d" % a)


@pytest.mark.parametrize("gnum,gk,expands", [(2, 3, False), (6, 1, True)])
def test_group_by_equals_the_twin_and_the_model(gnum, gk, expands):
    """seven groups and a result list of six: two groups are always among them, six only when the second walk has run"""
    r, q = _rows(200, 128, 128, 1), _rows(6, 128, 128, 3)
    g = H.build_graph(r.astype(np.float32), 5, 24, 7)
    c = G._case(g, q, np.arange(200) % 7, gnum, gk, 4, None)
    ms = G.model_of(c)
    assert all(m.expanded for m in ms) if expands else not any(m.expanded for m in ms)
    a, b = TG._search(_loaded(g, r, "l2"), c), TG._search(_loaded(g, r, "l2", "fp32"), c)
    assert [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b]
    TG._equals_model(a, ms, c)


def test_plumbing_and_refusals():
    from zvec_amd import _lib, index
    L, out, d = _lib.lib(), C.c_void_p(0x55), C.c_int(-1)
    typed, L2 = L.zvec_hip_hnsw_create_typed, _lib.METRIC_L2
    for create, dim, metric, want in ((typed, 0, L2, F.INVALID), (typed, 6, L2, F.INVALID), (typed, 4100, L2, F.UNSUPPORTED),
                                      (typed, 64, _lib.METRIC_COSINE, F.UNSUPPORTED), (typed, 64, _lib.METRIC_HAMMING, F.UNSUPPORTED),
                                      (L.zvec_hip_hnsw_create, 64, L2, F.UNSUPPORTED)):
        assert create(dim, _lib.DT_INT8, metric, 0, C.byref(out)) == want and out.value == 0x55, (dim, metric)
    for name in ("int8", np.int8):
        se = _searcher(4096, "ip", name)
        assert L.zvec_hip_hnsw_dtype(se._h, C.byref(d)) == 0 and d.value == 4 and se.np_dtype is np.int8 and se.info()["dim"] == 4096
        with pytest.raises(ValueError):
            index._dtype_of(name)
    assert se.load(np.zeros((3, 4092), np.int8), np.zeros((3, 2), np.uint32), np.zeros(3, np.uint32)) == F.MISMATCH


def _encode_ref(x, scale, bias, per_row):
    """the quantiser in numpy: fp32 operations one by one, then round half away from zero (exact in fp64)"""
    f32, mx = np.float32, np.abs(x).max(1)
    with np.errstate(divide="ignore"):
        s, fac = np.where(mx > 0, f32(127) / mx, f32(0)), np.where(mx > 0, mx / f32(127), f32(0))
    y = x * s[:, None] if per_row else np.clip((x + f32(bias)) * f32(scale), f32(-127), f32(127))
    assert y.dtype == s.dtype == fac.dtype == np.float32
    y = y.astype(np.float64)
    return np.copysign(np.floor(np.abs(y) + 0.5), y).astype(np.int8), fac


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("dim", [4, 100, 768])
def test_quantiser_equals_its_numpy_statement(dim, per_row, dev):
    """planted in rows 0 to 2: exact halves after scaling and, under (v + 1/4) * 2 (powers of two), values beyond both clamps.  Per
    row the largest magnitude is 254 = 127 * 2, so s = 1/2 exactly; row 2 is all negative, row 3 zero"""
    import torch
    import zvec_amd as zv
    halves = np.float32([0.5, -0.5, 1.5, -1.5, 126.5, -126.5])
    scale, bias = (None, 0.0) if per_row else (2.0, 0.25)
    plant = halves * 2 if per_row else np.concatenate([halves / 2 - np.float32(0.25), np.float32([1000, -1000])])
    x = np.random.default_rng([dim, per_row]).uniform(-254, 254, (12, dim)).astype(np.float32)
    m = min(dim - 1, plant.size)
    for row in (0, 1, 2):
        x[row, :m] = np.roll(plant, -3 * row)[:m]
    p32, p64 = x[:3, :m], x[:3, :m].astype(np.float64)
    y, exact = (p32 * np.float32(0.5), p64 * 0.5) if per_row else ((p32 + np.float32(bias)) * np.float32(scale), (p64 + bias) * scale)
    assert (y == exact).all() and set(halves) | (set() if per_row else {2000.5, -1999.5}) <= set(y.ravel())
    if per_row:
        x[:, dim - 1] = [254, -254] * 6
        x[2], x[3] = -np.abs(x[2]), 0
    want, fac = _encode_ref(x, scale, bias, per_row)
    if dev:
        ctx = zv.IndexContext(0)
        dx, do, df = torch.from_numpy(x).cuda(), torch.zeros(x.shape, dtype=torch.int8).cuda(), torch.full((12,), -1.0).cuda()
        torch.cuda.synchronize()
        ctx.int8_encode_dev(dx.data_ptr(), 12, dim, do.data_ptr(), scale, bias, per_row, df.data_ptr() if per_row else None)
        ctx.synchronize()
        got, gfac = do.cpu().numpy(), df.cpu().numpy()
    else:
        got, gfac = zv.int8_encode(x, per_row=True) if per_row else (zv.int8_encode(x, scale=scale, bias=bias), None)
    assert got.dtype == np.int8 and got.tobytes() == want.tobytes()
    assert not per_row or (gfac.tobytes() == fac.tobytes() and fac[3] == 0 and not got[3].any() and (x[2] < 0).all())


def test_c_example_runs(tmp_path):
    exe = str(tmp_path / "hnsw_int8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(F.ROOT, "include"), "-o", exe,
                           os.path.join(F.ROOT, "examples", "hnsw_int8.c"), "-L" + os.path.join(F.ROOT, "zvec_amd"), "-lzvec_hip",
                           "-Wl,-rpath," + os.path.join(F.ROOT, "zvec_amd")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, timeout=120)
    assert out.returncode == 0 and "hnsw_int8 ok" in out.stdout.decode(), out.stdout.decode()

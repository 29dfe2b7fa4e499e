"""Group-by search over sparse rows on the GPU (zvec_hip_sparse_search_grouped, zvec_hip_sparse_search_grouped_by_ids) against
tests/sparse_group_ref.py, through the C ABI, for both value types and with "sparse_group_rows" at 0 (every score dump by the
lane = query scan) and at 64 (every sub-batch of up to 64 queries by the wave-per-row kernel).  Integer cases are held bit for bit;
the Gaussian case inside the band B = (m + 1) * 2^-23 * A of tests/sparse_ref.py."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_group_ref as G  # noqa: E402
import sparse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, OUT_OF_RANGE, INVALID = -12, -17, -31
FLT_MAX = float(np.finfo(np.float32).max)
DTYPES = ["fp32", "fp16"]
NP = {"fp32": np.float32, "fp16": np.float16}


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _lib():
    from zvec_amd import _lib as L
    return L.lib()


@contextlib.contextmanager
def _group_rows(value):
    """"sparse_group_rows" set to `value`, the previous value restored afterwards"""
    L = _lib()
    before = C.c_int(-1)
    assert L.zvec_hip_get_option(b"sparse_group_rows", C.byref(before)) == 0
    assert L.zvec_hip_set_option(b"sparse_group_rows", value) == 0
    try:
        yield
    finally:
        assert L.zvec_hip_set_option(b"sparse_group_rows", before.value) == 0


_INDEXES = {}


def _index(kind, n, nq, dtype):
    """one index per case and value type, shared (nothing below changes it); keys = position * 3 + 7, appended in two pieces"""
    key = (kind, n, nq, dtype)
    if key not in _INDEXES:
        import zvec_amd as zv
        counts, idx, val = G.make_case(kind, n, nq)[0]
        off = R.offsets(counts)
        se = zv.HipFlatSparseStreamer(dtype=dtype)
        keys = _key_of(n)
        for a, b in ((0, n // 2), (n // 2, n)):
            if b > a:
                assert se.add_batch(counts[a:b], idx[off[a]:off[b]], val[off[a]:off[b]], keys[a:b]) == 0
        assert se.count() == n
        _INDEXES[key] = (se, se.create_context())
    return _INDEXES[key]


def _key_of(n):
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)


def _words_of(mask):
    w = np.zeros((mask.size + 63) // 64, np.uint64)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(w, idx // 64, np.uint64(1) << (idx % 64).astype(np.uint64))
    return w


def _outputs(count, gnum, gk, fill=None):
    shapes = [((count, gnum), np.uint32), ((count,), np.uint32), ((count, gnum, gk), np.uint64), ((count, gnum, gk), np.float32),
              ((count, gnum), np.uint32)]
    return tuple(np.zeros(s, t) if fill is None else np.full(s, fill, t) for s, t in shapes)


def _search(index, dtype, queries, gof, ng, gnum, gk, threshold=None, exclude=None, lists=None):
    """the C ABI call: (rc, (groups, ngroups, keys, scores, counts))"""
    se, ctx = index
    c, i, v = queries
    c = np.ascontiguousarray(c, np.uint32)
    i = np.ascontiguousarray(i, np.uint32)
    v = np.ascontiguousarray(v).astype(NP[dtype])
    assert np.array_equal(v.astype(np.float32), np.asarray(queries[2], np.float32)), "the case's values are not of the index's type"
    count = len(c)
    out = _outputs(count, gnum, gk)
    gof = np.ascontiguousarray(gof, np.uint32)
    ex = None if exclude is None else _words_of(np.asarray(exclude, bool))
    thr = FLT_MAX if threshold is None else threshold
    L = _lib()
    if lists is None:
        rc = L.zvec_hip_sparse_search_grouped(se._h, ctx._h, _ptr(c), _ptr(i), _ptr(v), count, _ptr(gof), ng, gnum, gk, thr, _ptr(ex),
                                              *[_ptr(a) for a in out])
    else:
        ids = np.concatenate([np.asarray(a, np.uint32) for a in lists] + [np.zeros(1, np.uint32)]).astype(np.uint32)
        offs = np.zeros(count + 1, np.uint32)
        offs[1:] = np.cumsum([len(a) for a in lists])
        rc = L.zvec_hip_sparse_search_grouped_by_ids(se._h, ctx._h, _ptr(c), _ptr(i), _ptr(v), count, _ptr(ids), _ptr(offs), _ptr(gof),
                                                     ng, gnum, gk, thr, _ptr(ex), *[_ptr(a) for a in out])
    return rc, out


_WANT = {}


def _want(tag, case, which, gof, ng, gnum, gk, n, **kw):
    """the rendered reference of a leg, computed once per (tag, route) and shared by the value types and the two dumps"""
    key = (tag, gnum, gk)
    if key not in _WANT:
        r = G.group_reference(case[:5], gof, ng, gnum, gk, queries=list(which), **kw)
        _WANT[key] = (r, G.render(r["queries"], gnum, gk, _key_of(n)))
    return _WANT[key]


def _both_dumps(index, dtype, queries, gof, ng, gnum, gk, want, what, **kw):
    for w in (0, 64):
        with _group_rows(w):
            rc, got = _search(index, dtype, queries, gof, ng, gnum, gk, **kw)
        assert rc == 0, (what, w, rc)
        G.check_exact(want, got, "%s rows=%d (%d, %d)" % (what, w, gnum, gk))


# count 1: the query of 4096 pairs, and the query of 0 pairs alone; count 2: runs of 1 and 2 pairs; count 3: runs of 3, 0 and 1 pairs
# (at most 64 queries: the wave-per-row dump takes them, empty runs included); count 65: runs of 0, 1, 2, 3 and 4096 pairs, two
# query blocks (one sub-batch wider than 64: the lane = query dump at either setting)
QUERY_SETS = [(0,), (4,), (1, 2), (3, 4, 5), tuple(range(65))]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 2049])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_legs(dtype, n):
    case = G.make_case("int", n)
    gof, ng = case[5], case[6]
    index = _index("int", n, 65, dtype)
    for which in QUERY_SETS:
        queries = G.take_queries(case[1], which)
        for gnum, gk in G.ROUTES:
            _, want = _want(("int", n, which), case, which, gof, ng, gnum, gk, n)
            _both_dumps(index, dtype, queries, gof, ng, gnum, gk, want, "int n=%d count=%d" % (n, len(which)))


VAR_N, VAR_Q = 2049, (0, 1, 2, 3, 4, 7)            # (query 4 has no pairs: +0 everywhere, +inf where excluded)


@pytest.mark.parametrize("variant", ["exclude", "radius", "no_group", "zeros"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_variants(dtype, variant):
    kind = "zeros" if variant == "zeros" else "int"
    case = G.make_case(kind, VAR_N)
    gof, ng = case[5], case[6]
    rng = np.random.default_rng(11)
    kw = {}
    if variant == "exclude":
        mask = rng.random(VAR_N) < 0.3
        mask[128:192] = True                      # a whole 64-row store of the wave-per-row kernel
        mask[2048] = True                         # ... and the last, one-row one
        kw["exclude"] = mask
    elif variant == "radius":
        kw["threshold"] = -10.0
    elif variant == "no_group":
        gof = gof.copy()
        gof[::5] = ng
        gof[1::7] = 0xffffffff
    queries = G.take_queries(case[1], VAR_Q)
    index = _index(kind, VAR_N, 65, dtype)
    for gnum, gk in G.ROUTES:
        r, want = _want((variant, VAR_N), case, VAR_Q, gof, ng, gnum, gk, VAR_N, **kw)
        if variant == "radius":
            assert np.any(want[4][np.arange(gnum)[None, :] < want[1][:, None]] == 0) and want[4].max() > 0
        if variant == "zeros":
            assert np.mean(r["m"] == 0) > 0.9 and np.any(r["m"] > 0)
        _both_dumps(index, dtype, queries, gof, ng, gnum, gk, want, variant, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_by_ids(dtype):
    n = VAR_N
    case = G.make_case("int", n)
    gof, ng = case[5], case[6]
    rng = np.random.default_rng(12)
    mask = rng.random(n) < 0.2
    which = (0, 1, 2, 3, 4, 5, 6, 7, 17)
    lists = []
    for length in (0, 1, 63, 64, 65, 300, 0, 0, 70):      # (empty lists: offsets that repeat)
        a = rng.integers(0, n + 60, length)                # some positions beyond the rows
        if length >= 63:
            a[length // 2] = a[0]                          # a position listed twice
            a[-1] = a[1]
            a[3] = np.nonzero(mask)[0][length % 7]         # an excluded one for sure
        lists.append(a.astype(np.uint32))
    assert any((a >= n).any() for a in lists)
    queries = G.take_queries(case[1], which)
    index = _index("int", n, 65, dtype)
    for gnum, gk in G.ROUTES:
        for tag, kw in (("plain", {}), ("excluded", {"exclude": mask}), ("radius", {"exclude": mask, "threshold": -10.0})):
            _, want = _want(("ids", tag), case, which, gof, ng, gnum, gk, n, candidates=lists, **kw)
            rc, got = _search(index, dtype, queries, gof, ng, gnum, gk, lists=lists, **kw)
            assert rc == 0
            G.check_exact(want, got, "by ids %s (%d, %d)" % (tag, gnum, gk))


@pytest.mark.parametrize("dtype", DTYPES)
def test_real_leg(dtype):
    """Gaussian halves, 2049 rows, every fill route on both dumps: inside the band, and no more ambiguous than the CPU test allows"""
    n, nq = 2049, 4
    case = G.make_case("real", n, nq)
    gof, ng = case[5], case[6]
    index = _index("real", n, nq, dtype)
    pos_of_key = {int(k): p for p, k in enumerate(_key_of(n))}
    for gnum, gk in G.ROUTES:
        r, _ = _want(("real", n), case, range(nq), gof, ng, gnum, gk, n)
        amb, tot = G.ambiguity(r, gnum, gk)
        assert tot > 0 and amb * 4 <= tot, (gnum, gk, amb, tot)
        for w in (0, 64):
            with _group_rows(w):
                rc, (groups, ngroups, keys, scores, counts) = _search(index, dtype, case[1], gof, ng, gnum, gk)
            assert rc == 0
            ndiff = namb = 0
            for q in range(nq):
                d, a, _, gdiff, gamb = G.check_band(r, q, groups[q], ngroups[q], keys[q], scores[q], counts[q], gnum, gk, pos_of_key,
                                                    "real rows=%d (%d, %d) query %d" % (w, gnum, gk, q))
                ndiff, namb = ndiff + d, namb + a
                assert gamb or not gdiff, (w, gnum, gk, q, "the groups differ although the cut is not ambiguous")
            assert ndiff <= namb, (w, gnum, gk, ndiff, namb)


def test_errors_touch_no_output():
    n = 129
    case = G.make_case("int", n)
    gof, ng = np.ascontiguousarray(case[5], np.uint32), case[6]
    se, ctx = _index("int", n, 65, "fp32")
    L = _lib()
    qc, qi, qv = [np.ascontiguousarray(a) for a in G.take_queries(case[1], (1, 2, 3))]
    ids, offs = np.array([0, 5, 9], np.uint32), np.array([0, 1, 2, 3], np.uint32)
    SENT = 0x5a
    out = _outputs(3, 4, 4, SENT)
    clean = [a.copy() for a in out]
    po = [_ptr(a) for a in out]

    def full(h=se._h, counts=qc, indices=qi, values=qv, count=3, groups=gof, ngroups=ng, gnum=4, gk=4, outs=po):
        return L.zvec_hip_sparse_search_grouped(h, ctx._h, _ptr(counts), _ptr(indices), _ptr(values), count, _ptr(groups), ngroups, gnum,
                                                gk, FLT_MAX, None, *outs)

    def listed(h=se._h, counts=qc, indices=qi, values=qv, count=3, lids=ids, loffs=offs, groups=gof, ngroups=ng, gnum=4, gk=4, outs=po):
        return L.zvec_hip_sparse_search_grouped_by_ids(h, ctx._h, _ptr(counts), _ptr(indices), _ptr(values), count, _ptr(lids),
                                                       _ptr(loffs), _ptr(groups), ngroups, gnum, gk, FLT_MAX, None, *outs)

    for call in (full, listed):
        assert call(h=None) == INVALID
        assert call(groups=None) == INVALID
        assert call(counts=None) == INVALID
        assert call(indices=None) == INVALID
        assert call(values=None) == INVALID
        for j in range(5):
            assert call(outs=po[:j] + [None] + po[j + 1:]) == INVALID
        assert call(gnum=0) == INVALID
        assert call(gk=0) == INVALID
        assert call(ngroups=0) == INVALID
        assert call(gnum=5120) == UNSUPPORTED          # 5120 * 12 + 16 = 60 KiB + 16
        assert call(gk=3840) == UNSUPPORTED            # 3840 * 16 + 16 = 60 KiB + 16
        assert call(count=0) == 0
        down = qi.copy()
        down[1:3] = down[1:3][::-1]                    # query 1 (two pairs) descends
        assert qc[1] == 2 and call(indices=down) == INVALID
        same = qi.copy()
        same[2] = same[1]
        assert call(indices=same) == INVALID
        assert call(counts=np.array([1, 2, 4097], np.uint32)) == INVALID
    # more than 2^19 queries, and a candidate matrix of more than 2^32 - 1 cells (2^19 lists, the longest of 8193 entries)
    many = (1 << 19) + 1
    assert full(counts=np.zeros(many, np.uint32), count=many) == OUT_OF_RANGE
    assert listed(counts=np.zeros(many, np.uint32), count=many, loffs=np.zeros(many + 1, np.uint32)) == OUT_OF_RANGE
    wide = np.full((1 << 19) + 1, 8193, np.uint32)
    wide[0] = 0
    assert listed(counts=np.zeros(1 << 19, np.uint32), count=1 << 19, lids=np.zeros(8193, np.uint32), loffs=wide) == OUT_OF_RANGE
    assert listed(loffs=None) == INVALID
    assert listed(lids=None) == INVALID
    assert listed(loffs=np.array([1, 1, 2, 3], np.uint32)) == INVALID
    assert listed(loffs=np.array([0, 2, 1, 3], np.uint32)) == INVALID
    for a, b in zip(out, clean):
        assert np.array_equal(a, b), "a refused call wrote to an output"
    assert full() == 0 and listed() == 0                # (the same arguments, unbroken, are served)
    assert L.zvec_hip_set_option(b"sparse_group_rows", 65) == INVALID and L.zvec_hip_set_option(b"sparse_group_rows", -1) == INVALID


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_index(dtype):
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer(dtype=dtype)
    index = (se, se.create_context())
    case = G.make_case("int", 1)
    queries = G.take_queries(case[1], (1, 2))
    for lists in (None, [np.array([0, 3], np.uint32), np.zeros(0, np.uint32)]):
        rc, got = _search(index, dtype, queries, np.zeros(1, np.uint32), 1, 3, 2, lists=lists)
        assert rc == 0 and got[1].tolist() == [0, 0] and not got[4].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_methods(dtype):
    n, which, gnum, gk = 129, (0, 1, 2, 3), 5, 3
    case = G.make_case("int", n)
    gof, ng = case[5], case[6]
    se, _ = _index("int", n, 65, dtype)
    key_of = _key_of(n)
    group_of_key = {int(k): "g%d" % gof[p] for p, k in enumerate(key_of)}
    # the context numbers the group ids in the order it meets them (IndexContext._groups_for): equal best scores rank by THAT number
    names = list(dict.fromkeys("g%d" % v for v in gof))
    dense = np.array([names.index("g%d" % v) for v in gof], np.uint32)
    qc, qi, qv = G.take_queries(case[1], which)
    banned = set(int(k) for k in key_of[::4])
    rng = np.random.default_rng(13)
    lists = [rng.integers(0, n, 40) for _ in which]
    for p_keys in (None, [key_of[a] for a in lists]):
        ctx = se.create_context()
        ctx.set_group_params(gnum, gk)
        ctx.set_group_by(lambda key: group_of_key[key])
        ctx.set_filter(lambda key: key in banned)
        # the methods that are not routed keep refusing a group context
        assert se.search_impl(qc, qi, qv, len(which), ctx) != 0
        if p_keys is None:
            assert se.group_by_search_impl(qc, qi, qv, len(which), ctx) == 0
        else:
            assert se.group_by_search_p_keys_impl(qc, qi, qv, p_keys, len(which), ctx) == 0
        exclude = np.zeros(n, bool)
        exclude[::4] = True
        r = G.group_reference(case[:5], dense, len(names), gnum, gk, exclude=exclude, candidates=None if p_keys is None else lists,
                              queries=list(which))
        for q, rq in enumerate(r["queries"]):
            got = ctx.group_result(q)
            assert [d.group_id() for d in got] == [names[g] for g, _, _ in rq["groups"]]
            for doc, (g, p, s) in zip(got, rq["groups"]):
                assert [x.key() for x in doc.docs()] == [int(k) for k in key_of[p]]
                assert [x.score() for x in doc.docs()] == [float(v) for v in s]

"""Group-by selection (zvk_group.hip.h, api_entry_group.inc.h) on every fill route against plain fp64 — run with -m gpu.

group_select fills the per-group lists by one of three device routes, chosen by lds1 = gnum*gk*8 + gnum*8 + 16, that is by
gnum*(gk+1):

  route  condition                       kernel
  A      gnum*(gk+1) <= 1918             group_fill_query_kernel<_,4>: 4 waves, then wave 0 folds the other three lists
  B      1918 < gnum*(gk+1) <= 7678      group_fill_query_kernel<_,1>
  C      gnum*(gk+1) > 7678              group_fill_kernel: one wave per (query, slot)

each in a HAS_CI=false form (dense scan, zvec_hip_flat_search_grouped) and a HAS_CI=true form (p_keys,
zvec_hip_flat_search_grouped_by_ids).  What each (gnum, gk) of CASES hits, and the legs that run it:

  (gnum, gk)  gnum*(gk+1)  route  what it hits                                         dense HAS_CI=false      p_keys HAS_CI=true
  (137, 13)   1918         A      largest of route A                                   exact, variants, real   exact
  (959, 1)    1918         A      largest of route A, gk = 1                           exact                   exact
  (138, 13)   1932         B      smallest of route B                                  exact                   exact
  (349, 21)   7678         B      largest of route B, gk <= 64                         exact, real             exact
  (22, 348)   7678         B      largest of route B, gk > 64: the chunked             exact, variants         exact
                                  sorted_insert and row write-out
  (350, 21)   7700         C      smallest of route C                                  exact, variants, real   exact
  (1200, 7)   9600         C      route C, many slots                                  exact                   exact
  (9, 900)    8109         C      route C, gk > 64                                     exact                   exact
  (3, 2)      9            A      query slices (q0 != 0) at 32768 queries              slicing run 1           slicing run 2
  (4, 3)      16           A      query slices of the 1 GiB score matrix, 2^20+37 rows slicing run 3           -

"exact": integers in [-6, 6] (exact scores, many ties), L2 fp32 / InnerProduct fp32 / L2 fp16, at 1, 63, 511, 512, 513, 2047,
2049 and 12289 rows (the 64-lane, 512-candidate = one wave's run, and 2048-candidate = four waves' stride boundaries); every
list held exactly by tests/util.py check_groups_exact.  The small row counts have fewer admissible groups than gnum.
"variants": exclusion bitset, radius, rows with group_of >= ngroups, holes made by add_with_id.  "real": Gaussian data and the
same +3.0, membership and scores inside the derived bands of tests/util.py group_reference / check_groups_band.
The C ABI is driven directly (zvec_amd._lib on the handle of a HipFlatStreamer), so the test sets group_of, ngroups and the
exclusion words itself."""
import ctypes as C

import numpy as np
import pytest

from tests import util as U

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
DIM = 40                                                  # padded scan width 64
ROWS = (1, 63, 511, 512, 513, 2047, 2049, 12289)
NMAX = ROWS[-1]
# (gnum, gk) -> ngroups: with the skewed group sizes of _group_of some groups are larger than gk and some are not
CASES = {(137, 13): 400, (959, 1): 1500, (138, 13): 400, (349, 21): 400, (22, 348): 30, (350, 21): 400, (1200, 7): 1500, (9, 900): 12}
ROUTE = {(137, 13): "A", (959, 1): "A", (138, 13): "B", (349, 21): "B", (22, 348): "B", (350, 21): "C", (1200, 7): "C", (9, 900): "C"}
VARIANT_CASES = [(137, 13), (22, 348), (350, 21)]         # one per route
KINDS = [("SquaredEuclidean", "fp32"), ("InnerProduct", "fp32"), ("SquaredEuclidean", "fp16")]
NQ = 7


def test_case_table_matches_the_dispatch():
    """the table above restates fill_waves of group_select; this holds the restatement to the formula"""
    for (gnum, gk), route in ROUTE.items():
        lds1 = gnum * gk * 8 + gnum * 8 + 16
        assert ("A" if lds1 * 4 <= 60 * 1024 else "B" if lds1 <= 60 * 1024 else "C") == route
    for (gnum, gk) in [(137, 13), (959, 1), (349, 21), (22, 348)]:          # the largest of their routes: one more slot leaves it
        lds1 = (gnum + 1) * gk * 8 + (gnum + 1) * 8 + 16
        assert lds1 * (4 if ROUTE[(gnum, gk)] == "A" else 1) > 60 * 1024


def _npdt(dtype):
    return np.float16 if dtype == "fp16" else np.float32


def _words(bits):
    b = np.zeros((len(bits) + 63) // 64 * 64, np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def _group_of(rng, n, ngroups):
    """group sizes fall from ~n / ngroups^(1/3) to ~n / (3 ngroups)"""
    return np.minimum((ngroups * rng.random(n) ** 3).astype(np.uint32), ngroups - 1)


_cache = {}


def _index(metric, dtype, n, holes=False, dim=DIM, integer=True, offset=0.0):
    """(streamer, rows, keys per position, hole mask) — seeded, built once per module.  holes: the index is filled through
    add_with_id (key = position) and every 5th position but the last stays a hole."""
    import zvec_amd
    key = (metric, dtype, n, holes, dim, integer, offset)
    if key not in _cache:
        rng = np.random.default_rng([11, n, dim, int(holes), int(integer)])
        if integer:
            base = rng.integers(-6, 7, (n, dim)).astype(_npdt(dtype))
        else:
            base = (rng.standard_normal((n, dim)) + offset).astype(_npdt(dtype))
        st = zvec_amd.HipFlatStreamer(dim, metric, dtype=dtype)
        hole = np.zeros(n, bool)
        if holes:
            hole[:n - 1:5] = n > 1
            ids = np.nonzero(~hole)[0].astype(np.uint32)
            assert st.add_with_id_batch(ids, base[ids]) == 0
            keys = np.arange(n, dtype=np.uint64)
        else:
            keys = (rng.permutation(3 * n)[:n] + 5).astype(np.uint64)
            assert st.add_batch(base, keys) == 0
        assert st.count() == n
        _cache[key] = (st, base, keys, hole)
    return _cache[key]


def _queries(seed, nq, dim, dtype, integer=True, offset=0.0):
    rng = np.random.default_rng([13, seed, nq, dim])
    if integer:
        return rng.integers(-6, 7, (nq, dim)).astype(_npdt(dtype))
    return (rng.standard_normal((nq, dim)) + offset).astype(_npdt(dtype))


def _search(st, q, of, ngroups, gnum, gk, threshold=FLT_MAX, exclude=None, lists=None):
    """the C ABI call; lists: per query the candidate positions (p_keys form).  Returns groups [nq][gnum], ngroups [nq],
    keys / scores [nq][gnum][gk], counts [nq][gnum]."""
    from zvec_amd import _lib
    L = _lib.lib()
    nq = len(q)
    q = np.ascontiguousarray(q)
    of = np.ascontiguousarray(of, np.uint32)
    assert of.size == st.count()
    groups = np.full((nq, gnum), 0xdeadbeef, np.uint32)
    ngr = np.full(nq, 0xdeadbeef, np.uint32)
    keys = np.zeros((nq, gnum, gk), np.uint64)
    scores = np.zeros((nq, gnum, gk), np.float32)
    counts = np.full((nq, gnum), 0xdeadbeef, np.uint32)
    ex = None if exclude is None else _words(exclude)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    if lists is None:
        rc = L.zvec_hip_flat_search_grouped(st._h, None, C.c_void_p(q.ctypes.data), nq, p(of, u32p), ngroups, gnum, gk, C.c_float(threshold),
                                            p(ex, u64p), p(groups, u32p), p(ngr, u32p), p(keys, u64p), p(scores, f32p), p(counts, u32p))
    else:
        offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.zeros(1, np.uint32)]))
        rc = L.zvec_hip_flat_search_grouped_by_ids(st._h, None, C.c_void_p(q.ctypes.data), nq, p(ids, u32p), p(offs, u32p), p(of, u32p),
                                                   ngroups, gnum, gk, C.c_float(threshold), p(ex, u64p), p(groups, u32p), p(ngr, u32p),
                                                   p(keys, u64p), p(scores, f32p), p(counts, u32p))
    assert rc == 0
    return groups, ngr, keys, scores, counts


def _check_exact(ref, out, gk, key_of, threshold=None, what="", sel=None):
    groups, ngr, keys, scores, counts = out
    for j, rq in enumerate(ref["queries"]):
        qi = j if sel is None else sel[j]
        U.check_groups_exact(rq, groups[qi], ngr[qi], keys[qi], scores[qi], counts[qi], gk, key_of,
                             threshold=None if threshold is None else threshold, what="%s query %d" % (what, qi))


def _cut_and_uncut(ref, gk):
    """does some listed group have more than gk members, and some listed group not"""
    sizes = [len(rq["order"][g][0]) for rq in ref["queries"] for g, _, _ in rq["groups"]]
    return any(s > gk for s in sizes), any(s <= gk for s in sizes)


# ---- exact leg ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dtype", KINDS)
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "%dx%d" % c)
def test_exact_dense_all_row_counts(case, metric, dtype):
    (gnum, gk), ngroups = case, CASES[case]
    for n in ROWS:
        st, base, keys, _ = _index(metric, dtype, n)
        q = _queries(n, NQ, DIM, dtype)
        of = _group_of(np.random.default_rng([17, n, ngroups]), n, ngroups)
        ref = U.group_reference(base, q, of, ngroups, gnum, gk, metric)
        if n == NMAX:
            cut, uncut = _cut_and_uncut(ref, gk)
            assert cut and uncut, "badly chosen inputs: cut lists %r, uncut lists %r" % (cut, uncut)
        if n == 1:
            assert all(len(rq["groups"]) < gnum for rq in ref["queries"]), "badly chosen inputs: no query short of groups"
        _check_exact(ref, _search(st, q, of, ngroups, gnum, gk), gk, keys, what="%r n=%d %s %s" % (case, n, metric, dtype))


@pytest.mark.parametrize("metric,dtype", KINDS)
@pytest.mark.parametrize("case", VARIANT_CASES, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("variant", ["exclude", "radius", "nogroup", "holes"])
def test_exact_dense_variants(variant, case, metric, dtype):
    (gnum, gk), ngroups = case, CASES[case]
    for n in (513, NMAX):
        st, base, keys, hole = _index(metric, dtype, n, holes=variant == "holes")
        q = _queries(n + 1, NQ, DIM, dtype)
        rng = np.random.default_rng([19, n, ngroups])
        of = _group_of(rng, n, ngroups)
        what = "%s %r n=%d %s %s" % (variant, case, n, metric, dtype)
        exclude = threshold = None
        if variant == "exclude":
            exclude = rng.random(n) < 0.4
            exclude[(of % 7) == 3] = True                                 # whole groups go
        elif variant == "nogroup":
            # numbers in [ngroups, 2 ngroups): such a row must never appear, and its number indexes nothing
            sel = rng.random(n) < 0.3
            of[sel] = ngroups + rng.integers(0, ngroups, int(sel.sum())).astype(np.uint32)
        elif variant == "radius":
            # below the best of query 0's last listed group (it is listed with no document), above the best of its first
            free = U.group_reference(base, q, of, ngroups, gnum, gk, metric)
            b = free["queries"][0]["bests"][0][:gnum]
            assert b[-1] > b[0], "badly chosen inputs: query 0's groups share one best score"
            threshold = float(np.float32(0.5 * (b[-1] + b[len(b) // 2])))
            if threshold >= b[-1]:
                threshold = float(b[-1]) - 0.5
        ref = U.group_reference(base, q, of, ngroups, gnum, gk, metric, threshold=threshold, exclude=hole if variant == "holes" else exclude)
        if variant == "radius" and n == NMAX:
            got_n = [len(p) for rq in ref["queries"] for _, p, _ in rq["groups"]]
            full_n = [min(gk, len(rq["order"][g][0])) for rq in ref["queries"] for g, _, _ in rq["groups"]]
            assert any(a == 0 for a in got_n) and any(0 < a < f for a, f in zip(got_n, full_n)), "badly chosen radius"
        out = _search(st, q, of, ngroups, gnum, gk, threshold=FLT_MAX if threshold is None else threshold, exclude=exclude)
        _check_exact(ref, out, gk, keys, threshold=threshold, what=what)
        if variant == "nogroup":
            ng = out[1]
            assert all(int(g) < ngroups for qi in range(NQ) for g in out[0][qi, :ng[qi]])


# ---- p_keys leg ---------------------------------------------------------------------------------------------------------------------
def _pkey_lists(rng, n, nq, hole, exclude):
    """lists of differing lengths: [0] empty, [1] one id, [2] a long one naming ids >= n, excluded ids, holes and one position
    twice; the rest of random lengths, up to more than four waves' stride"""
    lists = [np.zeros(0, np.uint32), np.array([n - 1], np.uint32)]
    live = np.nonzero(~hole & ~exclude)[0]
    long_ = np.concatenate([rng.choice(n, min(n, 3000), replace=False), [n, n + 70, 0xfffffffe, U.IDX_NONE], np.nonzero(hole)[0][:50],
                            np.nonzero(exclude)[0][:50], live[:3], live[:1]]).astype(np.uint32)
    lists.append(long_[rng.permutation(long_.size)])
    for _ in range(nq - 3):
        m = int(rng.integers(1, max(2, min(n, 5000))))
        lists.append(rng.choice(n + 20, m, replace=False).astype(np.uint32))
    return lists


@pytest.mark.parametrize("metric,dtype", KINDS)
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "%dx%d" % c)
def test_exact_p_keys(case, metric, dtype):
    (gnum, gk), ngroups = case, CASES[case]
    for n in (513, NMAX):
        st, base, keys, hole = _index(metric, dtype, n, holes=True)
        q = _queries(n + 2, NQ, DIM, dtype)
        rng = np.random.default_rng([23, n, ngroups])
        of = _group_of(rng, n, ngroups)
        exclude = rng.random(n) < 0.2
        exclude[n - 1] = False                                            # (the one id of list 1: live)
        assert not hole[n - 1]
        lists = _pkey_lists(rng, n, NQ, hole, exclude)
        ref = U.group_reference(base, q, of, ngroups, gnum, gk, metric, exclude=hole | exclude, candidates=lists)
        assert len(ref["queries"][0]["groups"]) == 0 and len(ref["queries"][1]["groups"]) == 1
        out = _search(st, q, of, ngroups, gnum, gk, exclude=exclude, lists=lists)
        assert out[1][0] == 0, "an empty list must return no group"
        _check_exact(ref, out, gk, keys, what="p_keys %r n=%d %s %s" % (case, n, metric, dtype))


# ---- real-valued leg ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
@pytest.mark.parametrize("offset", [0.0, 3.0], ids=["centred", "plus3"])
@pytest.mark.parametrize("case", [(137, 13), (349, 21), (350, 21)], ids=lambda c: "%dx%d" % c)
def test_real_valued_membership_and_scores(case, offset, metric):
    """Gaussian rows and queries (offset 3.0: norms dwarf distances).  The caps are conditions on the inputs: at most 1 % (5 %
    with the offset) of the cut lists ambiguous, and the group cut unambiguous for at least half the queries."""
    (gnum, gk), ngroups, n, nq = case, 400, NMAX, 9
    st, base, keys, _ = _index(metric, "fp32", n, integer=False, offset=offset)
    # (the seed of the queries is fixed so that the last condition holds: computed on the fp64 reference alone, the L2 group cut
    # at rank 137 of 400 with the offset is ambiguous for 2-8 of 9 random queries, for 2 of these)
    q = _queries(45, nq, DIM, "fp32", integer=False, offset=offset)
    of = np.random.default_rng([29, n, ngroups]).integers(0, ngroups, n).astype(np.uint32)      # groups of ~31 rows: every list is cut
    ref = U.group_reference(base, q, of, ngroups, gnum, gk, metric)
    groups, ngr, gkeys, scores, counts = _search(st, q, of, ngroups, gnum, gk)
    pos_of_key = {int(k): i for i, k in enumerate(keys)}
    ndiff = namb = ncut = gclear = 0
    for qi in range(nq):
        d, a, c, gdiff, gamb = U.check_groups_band(ref, qi, groups[qi], ngr[qi], gkeys[qi], scores[qi], counts[qi], gnum, gk, pos_of_key,
                                                   metric, DIM, what="%r +%g %s query %d" % (case, offset, metric, qi))
        ndiff, namb, ncut = ndiff + d, namb + a, ncut + c
        assert gamb or not gdiff, "query %d: the listed groups differ from the fp64 ones and the cut is not ambiguous" % qi
        gclear += not gamb
    print("%r +%g %s: %d cut lists, %d ambiguous, %d differ; group cut unambiguous for %d of %d queries" % (
        case, offset, metric, ncut, namb, ndiff, gclear, nq))
    assert ndiff <= namb, "%d lists differ from the fp64 set, only %d are ambiguous" % (ndiff, namb)
    assert ncut > 0 and namb <= (0.05 if offset else 0.01) * ncut, "badly chosen inputs: %d of %d cut lists ambiguous" % (namb, ncut)
    assert 2 * gclear >= nq, "badly chosen inputs: the group cut is ambiguous for %d of %d queries" % (nq - gclear, nq)


# ---- slicing leg --------------------------------------------------------------------------------------------------------------------
def _near(boundaries, count, width=3):
    s = {0, count - 1}
    for b in boundaries:
        s.update(range(max(0, b - width), min(count, b + width)))
    return sorted(s)


@pytest.mark.parametrize("p_keys", [False, True], ids=["dense", "p_keys"])
def test_slices_at_32768_queries(p_keys):
    """32770 queries: both entry points slice at 32768.  Every query has its own data, so a result written at, or read from,
    the wrong q0 cannot pass; the reference is computed for query 0, the last one and three on each side of the boundary."""
    count, n, dim, gnum, gk, ngroups = 32770, 200, 8, 3, 2, 10
    st, base, keys, _ = _index("SquaredEuclidean", "fp32", n, dim=dim)
    q = _queries(41, count, dim, "fp32")
    rng = np.random.default_rng(43)
    of = rng.integers(0, ngroups, n).astype(np.uint32)
    lists = [rng.integers(0, n, int(m)).astype(np.uint32) for m in rng.integers(1, 5, count)] if p_keys else None
    out = _search(st, q, of, ngroups, gnum, gk, lists=lists)
    sel = _near([32768], count)
    ref = U.group_reference(base, q[sel], of, ngroups, gnum, gk, candidates=None if lists is None else [lists[i] for i in sel])
    _check_exact(ref, out, gk, keys, what="slices p_keys=%r" % p_keys, sel=sel)


def test_slices_of_the_score_matrix():
    """2^20 + 37 rows, 600 queries: the dense score matrix is capped at 1 GiB, which gives three slices.  The slice width is
    not recomputed here: the checked queries 0-2, 250-262, 505-520, 597-599 cover the boundaries for any tile width 64-512."""
    count, n, dim, gnum, gk, ngroups = 600, (1 << 20) + 37, 8, 4, 3, 50
    st, base, keys, _ = _index("SquaredEuclidean", "fp32", n, dim=dim)
    q = _queries(47, count, dim, "fp32")
    of = np.random.default_rng(53).integers(0, ngroups, n).astype(np.uint32)
    out = _search(st, q, of, ngroups, gnum, gk)
    sel = list(range(0, 3)) + list(range(250, 263)) + list(range(505, 521)) + list(range(597, 600))
    ref = U.group_reference(base, q[sel], of, ngroups, gnum, gk)
    _check_exact(ref, out, gk, keys, what="1 GiB slices", sel=sel)
    del _cache[("SquaredEuclidean", "fp32", n, False, dim, True, 0.0)]

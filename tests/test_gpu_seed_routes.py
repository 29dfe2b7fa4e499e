"""Seeded admission bounds on every seeded flat route against fp64 — run with -m gpu.

Every store has 262 144 rows, the smallest size flat_scan_prepared seeds.  Each case names its route (tests/seed_ref.py CASES: the
dispatch restated) and the search must report that very route word (zvec_hip_ctx_last_route) before its answer is compared with the
fp64 reference of seed_ref.reference.  A bound that is too tight raises no error: the query comes back short, or without a true
neighbour — which is what every case here would show.

  offset    1000 + small integers, the k nearest rows planted inside the seeding prefix (layouts of seed_ref.layout_positions); the
            norms are ~1e6 dim, so the planted rows' selection scores differ between tile shapes by whole ulps of the norms while
            their distances differ by 0..2: the case the slack of the seeding kernels exists for.  The fixture's preconditions
            (fp64 top-k == the planted rows, runner-up further than twice the select band) are asserted before every search.
  exact     integers in [-6, 6]: exact scores, ties at the k-th place inside and outside the prefix; bit-exact, keys by (score, position)
  gaussian  unit normal rows, queries = prefix rows + 0.05 noise; the bands of DESIGN §4

Cosine runs on gaussian rows only (cases 6 and 11): the offset fixture cannot be stated for it — normalising rows of 1000 + [0, 16)
leaves 1 - cos ~ 1e-6 between ANY two rows, inside the 4e-6 band, so no planted set is decided by the reference.  Nor is there an
exact kind under cosine: integer rows are no longer integers once divided by their norms, so no score is exact and the kind would
only repeat the gaussian one with a coarser spread.

Host memory: the unplanted rows of a store are built once per module by the `bg` fixture, which keeps at most ONE array of the
768-dim store (0.8 GB) at a time and frees everything at module teardown; the tests are ordered metric-major so that each of those
arrays is built once."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import seed_ref as R
from tests.util import tie_tolerant_compare

pytestmark = pytest.mark.gpu
L2, IP = "SquaredEuclidean", "InnerProduct"


@pytest.fixture(scope="module")
def zv():
    import zvec_amd
    return zvec_amd


@pytest.fixture(scope="module")
def bg():
    """(store, kind, metric) -> the unplanted rows of a store: built once, never changed (planted rows are put in and taken out
    again).  One 768-dim array at a time; everything is released when the module is done."""
    cache = {}

    def get(store, kind, metric, transform=None):
        key = (store, kind, metric if kind == "offset" or transform else L2)
        if key not in cache:
            if store == "D768":
                for other in [o for o in cache if o[0] == "D768"]:
                    del cache[other]
            dim, f16 = R.STORES[store]
            rows = R.background(kind, L2 if transform else key[2], dim, f16, seed=1)
            cache[key] = transform(rows) if transform else rows
        return cache[key]
    yield get
    cache.clear()


class _Planted:
    """rows `pos` of `base` replaced for the length of a with-block"""

    def __init__(self, base, pos, rows):
        self.base, self.pos, self.rows = base, pos, rows

    def __enter__(self):
        self.save = self.base[self.pos].copy()
        self.base[self.pos] = self.rows.astype(self.base.dtype)
        return self.base

    def __exit__(self, *a):
        self.base[self.pos] = self.save


def _search(zv, base, metric, f16, q, k, drop=None, thr=None, se=None):
    se = se or zv.HipFlatSearcher(base.shape[1], metric, dtype="fp16" if f16 else "fp32")
    if se.count() == 0:
        assert se.load(base) == 0                                             # keys = positions
    ctx = se.create_context()
    ctx.set_topk(k)
    if drop is not None:
        ctx.set_exclude_bitset(O.pack_bits(drop))
    if thr is not None:
        ctx.set_threshold(thr)
    assert se.search_impl(q, len(q), ctx) == 0
    return se, ctx.keys.copy(), ctx.scores.copy(), ctx.counts.copy(), ctx.last_route()


def _assert_route(got, want, what):
    assert got == want, "%s: ran %s, expected %s" % (what, R.describe(got), R.describe(want))


def _norm_max(base, keys_a, keys_b, counts, d):
    """per query the largest |b|^2 among the rows either side returned"""
    out = np.zeros(len(counts))
    for i in range(len(counts)):
        p = np.unique(np.concatenate([keys_a[i, :counts[i]], keys_b[i, :counts[i]]]).astype(np.int64))
        out[i] = (base[p].astype(np.float64)[:, :d] ** 2).sum(1).max() if p.size else 0.0
    return out


def _compare(base, q, metric, got, ref, what, exact=False):
    keys, scores, counts = got
    rk, rs, rc = ref
    assert np.array_equal(counts, rc), "%s: counts %r, reference %r" % (what, counts[counts != rc][:8], rc[counts != rc][:8])
    if exact:
        tie_tolerant_compare(keys, scores, counts, rk, rs, rc, what=what)
        for i in range(len(rc)):                                              # (score, position): the very rows of the reference
            assert np.array_equal(keys[i, :rc[i]], rk[i, :rc[i]]), "%s query %d: keys %r, by (score, position) %r" % (what, i, keys[i], rk[i])
        return
    d = base.shape[1] - (1 if metric == "Cosine" else 0)
    kw, _ = R.bands(_norm_max(base, keys, rk, rc, d), q, metric, cosine_dim=d if metric == "Cosine" else None)
    tie_tolerant_compare(keys, scores, counts, rk, rs, rc, what=what, **kw)


def _queries(kind, base, nq):
    """the queries of an exact or gaussian case; batches beyond 256 repeat a pool of 64 (the reference is taken once per distinct query)"""
    uniq = min(nq, 256 if nq <= 256 else R.QUERY_POOL)
    dt = base.dtype
    if kind == "exact":
        qu = np.random.default_rng([9, uniq, base.shape[1]]).integers(-6, 7, (uniq, base.shape[1])).astype(dt)
    else:
        rng = np.random.default_rng([10, uniq, base.shape[1]])
        qu = (base[rng.choice(R.SEED_ROWS, uniq, replace=False)].astype(np.float32)
              + 0.05 * rng.standard_normal((uniq, base.shape[1]), dtype=np.float32)).astype(dt)
    return qu, np.arange(nq) % uniq


def _run_offset(zv, bg, case, metric, layout, variant=None, radius=False):
    store, nq, k, share, want = R.CASES[case]
    f16 = R.STORES[store][1]
    what = "%s %s %s %s%s" % (case, store, metric, layout, " " + variant if variant else "")
    fx = R.offset_fixture(case, metric, layout, variant)
    drop, expect, pos, qmap = fx["drop"], fx["expect"], fx["pos"], fx["qmap"]
    bgrows = bg(store, "offset", metric)
    qu = fx["queries"].astype(bgrows.dtype)
    with _Planted(bgrows, pos, fx["planted"]) as base:
        rk, rs, rc, runner = R.reference(base, qu, k, metric, drop=drop, planted=pos, integer=True)
        bn = float((base[expect].astype(np.float64) ** 2).sum(1).max())
        _, band = R.bands(bn, qu, metric)
        R.check_planted_fixture(rk, rs, rc, runner, expect, band, k, what=what)     # the preconditions, again, on the very arrays searched
        kept = None if drop is None else int((~drop).sum())
        assert R.case_route(case, kept) == want
        q = qu[qmap]
        se, keys, scores, counts, route = _search(zv, base, metric, f16, q, k, drop)
        _assert_route(route, want, what)
        assert (counts == k).all(), "%s: %d queries came back short (fewest %d of %d)" % (what, (counts < k).sum(), counts.min(), k)
        bad = [i for i in range(nq) if set(keys[i].tolist()) != set(expect.tolist())]
        assert not bad, "%s: %d queries without the planted set, first %d: %r" % (what, len(bad), bad[0], keys[bad[0]])
        sel = np.arange(nq) if nq <= 256 else np.random.default_rng(4).choice(nq, 32, replace=False)
        _compare(base, q[sel], metric, (keys[sel], scores[sel], counts[sel]), (rk[qmap[sel]], rs[qmap[sel]], rc[qmap[sel]]), what)
        if radius:
            dim = base.shape[1]
            thr = R.offset_radius(metric, fx["centre"], dim)
            _, rs2, rc2, _ = R.reference(base, qu, k, metric, drop=drop, threshold=thr, integer=True)
            assert (np.abs(rs - thr) > band[:, None]).all() and (rc2 == k - 1).all()
            _, keys2, scores2, counts2, route2 = _search(zv, base, metric, f16, q, k, drop, thr=thr, se=se)
            _assert_route(route2, want, what + " radius between the groups")
            _compare(base, q, metric, (keys2, scores2, counts2), (rk, rs2, rc2), what + " radius between the groups")
            far = 1e9 if metric == L2 else 0.0                                # far above every planted score: nothing is cut
            _, keys3, scores3, counts3, route3 = _search(zv, base, metric, f16, q, k, drop, thr=far, se=se)
            _assert_route(route3, want, what + " radius far above")
            assert np.array_equal(counts3, counts) and np.array_equal(scores3, scores)
            assert all(set(keys3[i].tolist()) == set(expect.tolist()) for i in range(nq))


@pytest.mark.parametrize("case,layout", R.OFFSET_RUNS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_offset_rows_keep_their_planted_neighbours(zv, bg, metric, case, layout):
    _run_offset(zv, bg, case, metric, layout)


@pytest.mark.parametrize("case,layout,variant", R.PREFIX_RUNS)
@pytest.mark.parametrize("metric", [L2, IP])
def test_prefix_mostly_excluded(zv, bg, metric, case, layout, variant):
    """case 13, on case 11's shape: the prefix wholly excluded; exactly k - 1 of its rows kept; exactly k kept.  The host launches the
    prefix scan and seed_gtau_kernel in all three (same route word); in the first two the prefix list stays short and the kernel
    leaves the threshold, in the third the single full list's k-th score (+ slack) is the bound and must admit the row it came from."""
    _run_offset(zv, bg, case, metric, layout, variant=variant)


@pytest.mark.parametrize("case", ["c06", "c11"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_radius_with_seeding(zv, bg, metric, case):
    """case 14: a radius between the near planted rows and the far one (further than the select band from both) cuts the lists to
    the reference's counts, k - 1; a radius far above them changes nothing.  Both start the shared bounds at the radius, not +inf."""
    _run_offset(zv, bg, case, metric, "spread", radius=True)


def _run_plain(zv, bg, case, kind, metric, oracle=None):
    store, nq, k, share, want = R.CASES[case]
    dim, f16 = R.STORES[store]
    what = "%s %s %s %s" % (case, store, metric, kind)
    base = bg(store, kind, metric)
    qu, qmap = _queries(kind, base, nq)
    if metric == "Cosine":
        base, qu = bg(store, kind, "Cosine", transform=oracle.cosine_transform), oracle.cosine_transform(qu)
    drop = R.drop_mask(share, seed=3) if share > 0 else None
    kept = None if drop is None else int((~drop).sum())
    assert R.case_route(case, kept) == want
    if nq > 256:                                                              # case 10: the full reference on 32 sampled queries
        sel = np.random.default_rng(4).choice(nq, 32, replace=False)
    else:
        sel = np.arange(nq)
    need = np.unique(qmap[sel])
    back = np.zeros(len(qu), np.int64)
    back[need] = np.arange(len(need))
    rk, rs, rc, _ = R.reference(base, qu[need], k, metric, drop=drop, integer=kind == "exact")
    q = qu[qmap]
    _, keys, scores, counts, route = _search(zv, base, metric, f16, q, k, drop)
    _assert_route(route, want, what)
    assert (counts == k).all(), "%s: %d queries came back short (fewest %d of %d)" % (what, (counts < k).sum(), counts.min(), k)
    if drop is not None:
        assert not drop[keys.astype(np.int64)].any(), what + ": an excluded row came back"
    r = back[qmap[sel]]
    _compare(base, q[sel], metric, (keys[sel], scores[sel], counts[sel]), (rk[r], rs[r], rc[r]), what, exact=kind == "exact")


@pytest.mark.parametrize("case", sorted(R.CASES))
@pytest.mark.parametrize("metric", [L2, IP])
def test_exact_rows_with_ties_at_the_kth_place(zv, bg, metric, case):
    _run_plain(zv, bg, case, "exact", metric)


@pytest.mark.parametrize("case", ["c02", "c06", "c08", "c11"])
@pytest.mark.parametrize("metric", [L2, IP])
def test_gaussian_rows_within_the_stated_bands(zv, bg, metric, case):
    _run_plain(zv, bg, case, "gaussian", metric)


@pytest.mark.parametrize("case", ["c06", "c11"])
def test_cosine_gaussian_rows_within_the_stated_band(zv, bg, oracle, case):
    _run_plain(zv, bg, case, "gaussian", "Cosine", oracle)

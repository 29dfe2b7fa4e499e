"""CPU checks of tests/seed_ref.py: the dispatch model against the case table of tests/test_gpu_seed_routes.py and at every boundary the
table sits next to, the model of seed_bound_kernel against a brute-force sort, and the preconditions of every planted fixture."""
import numpy as np
import pytest

from tests import seed_ref as R


def test_padded_sizes_land_on_the_intended_side_of_the_cache_limit():
    mib = {s: R.ROWS * R.padded_words(*R.STORES[s]) * 4 / 2.0 ** 20 for s in R.STORES}
    assert mib == {"R32": 32.0, "S32": 96.0, "S16": 96.0, "D768": 768.0}
    assert R.padded_words(*R.STORES["S16"]) // R.TILE_K == 3                  # three k-steps
    assert R.padded_words(73, False, cosine=True) == R.padded_words(72, False)  # the cosine twin of S32 scans the same width


def test_case_table_matches_the_dispatch_model_and_every_boundary_leaves_the_route():
    for name, (store, nq, k, share, want) in R.CASES.items():
        got = R.case_route(name)
        assert got == want, "%s: model %s, table %s" % (name, R.describe(got), R.describe(want))
    S = R.store_route
    seeded = lambda w: w >> R.SEED_SHIFT & 3
    # rows: one below 262 144 is not seeded, on every store and shape of the table
    for name, (store, nq, k, share, want) in R.CASES.items():
        dim, f16 = R.STORES[store]
        w = R.route_word(R.ROWS - 1, R.padded_words(dim, f16), f16, nq, k, share > 0, int((R.ROWS - 1) * (1 - share)))
        assert seeded(w) == 0 and w & R.SHAPE_MASK == want & R.SHAPE_MASK, name
    # k: 64 is seeded, 65 is not; 15 queries are not, 16 are
    assert seeded(S("S32", 65, 64)) and not seeded(S("S32", 65, 65))
    assert seeded(S("S32", 16, 10)) and not seeded(S("S32", 15, 10))
    # queries: 16 / 17 the 16-row shape against NG1, 32 / 33 NG1 against NG2, 64 / 65 NG2 against the 8-wave tile (streamed) ...
    assert [S("S32", n, 10) & R.SHAPE_MASK for n in (16, 17, 32, 33, 64, 65)] == [R.M16, R.NG1, R.NG1, R.NG2, R.NG2, R.SCAN8]
    # ... a cache-resident store stays on NG1 (k <= 8: no dense path) and takes the dense path from k = 9 while the scores fit 128 MiB
    assert [S("R32", n, 8) & R.SHAPE_MASK for n in (16, 17, 65, 300)] == [R.M16, R.NG1, R.NG1, R.NG1]
    assert S("R32", 64, 9) == R.DENSE and S("R32", 128, 9) == R.DENSE and S("R32", 129, 9) == R.NG1 | R.SEED_BOUND
    assert S("R32", 64, 8) == R.NG1 | R.SEED_BOUND
    # 255 / 256 queries: fp16 rows move to the 256 x 256 tile and its 16 384-row prefix; fp32 rows do not; k = 12 does not fit it
    assert S("S16", 255, 10) & R.SCAN8 and S("S16", 256, 10) & R.SCAN256 and S("S32", 256, 10) & R.SCAN8
    assert S("S16", 256, 11) & R.SCAN256 and S("S16", 256, 12) & R.SCAN8
    dim, f16 = R.STORES["S16"]
    assert R.prefix_rows(R.ROWS, 96, True, 256, 10) == 16384 and R.prefix_rows(R.ROWS, 96, True, 255, 10) == 4096
    # the prefix dump: 16 384 rows x 4096 queries are exactly 256 MiB (seed_bound_kernel), 4097 pass it (prefix scan with lists)
    assert seeded(S("S16", 4096, 10)) == 1 and seeded(S("S16", 4097, 10)) == 2
    # filters: a wide batch gathers from 90 % kept down, a small one compacts from 50 % down; above, the exclusion variants run
    n = R.ROWS
    assert S("S32", 65, 10, True, int(0.9 * n) + 1) == R.CASES["c11"][4]
    assert S("S32", 65, 10, True, int(0.9 * n)) == R.GATHER
    assert S("S32", 40, 10, True, n // 2 + 1) == R.CASES["c12"][4]
    assert S("S32", 40, 10, True, n // 2) == R.COMPACT | R.DENSE              # (the copy is 48 MiB: cache resident, k > 8)
    assert S("D768", 40, 10, True, n // 2) == R.COMPACT | R.NG2
    assert S("S32", 72, 10, True, n - 1) & R.EXCL


def test_lds_formulas_at_the_limits_the_dispatch_uses():
    assert R.scan_lds_bytes(1, 64) == 58256 and R.scan8_lds_bytes(65) == 135696 == R.scan_lds_bytes(4, 65)
    assert R.scan256_lds_bytes(11) <= R.LDS_LIMIT < R.scan256_lds_bytes(12)
    assert R.pick_ng(65, 10) == 4 and R.pick_ng(64, 10) == 2 and R.pick_ng(32, 10) == 1 and R.pick_ng(300, 5000) == 0


def _true_kth(row, k):
    s = np.sort(row)
    return s[k - 1] if k <= len(s) else np.inf


def test_seed_bound_model_never_undercuts_the_true_kth_and_meets_it_when_the_best_sit_in_different_shares():
    rng = np.random.default_rng(5)
    for k in (1, 2, 10, 64):
        for n in (4096, 16384, 300, 256, 255):
            for _ in range(6):
                row = rng.standard_normal(n)
                row[rng.random(n) < 0.3] = np.inf                             # excluded columns
                assert R.seed_bound_model(row, k) >= _true_kth(row, k)
        # one share: every finite score in one thread's columns -> one minimum, no bound for k >= 2
        row = np.full(4096, np.inf)
        row[R.layout_positions("one_share", 10)] = np.arange(10.0)
        assert R.seed_bound_model(row, k) == (0.0 if k == 1 else np.inf) >= _true_kth(row, k)
        # k - 1 finite scores: no bound
        row = np.full(4096, np.inf)
        row[R.layout_positions("spread", max(k - 1, 1))[:k - 1]] = 1.0
        assert R.seed_bound_model(row, k) == np.inf
        # the k best in k different shares: the bound IS the k-th
        row = 10.0 + rng.random(4096)
        pos = R.layout_positions("spread", k)
        row[pos] = np.arange(k) * 0.125
        assert R.seed_bound_model(row, k) == _true_kth(row, k) == (k - 1) * 0.125
        # ... in one tile (one_chunk: odd columns of one tile, still distinct shares)
        row = 10.0 + rng.random(4096)
        row[R.layout_positions("one_chunk", k)] = np.arange(k) * 0.125
        assert R.seed_bound_model(row, k) == (k - 1) * 0.125


def test_layouts_are_what_they_say():
    for k in (1, 8, 10, 64):
        R.layout_positions("spread", k)
        R.layout_positions("one_chunk", k)
        R.layout_positions("behind", k)
    for k in (1, 8, 10, 13):
        R.layout_positions("one_share", k)
        assert (R.layout_positions("late", k) >= R.SEED_ROWS).all()


def test_reference_takes_the_k_best_by_score_then_position():
    rng = np.random.default_rng(2)
    base = rng.integers(-2, 3, (3000, 5)).astype(np.float32)
    q = rng.integers(-2, 3, (7, 5)).astype(np.float32)
    drop = rng.random(3000) < 0.3
    for metric in ("SquaredEuclidean", "InnerProduct"):
        keys, scores, counts, _ = R.reference(base, q, 9, metric, drop=drop, integer=True, chunk=700)
        b, qq = base.astype(np.float64), q.astype(np.float64)
        full = ((qq[:, None] - b[None]) ** 2).sum(-1) if metric == "SquaredEuclidean" else -(qq @ b.T)
        full[:, drop] = np.inf
        want = np.argsort(full, axis=1, kind="stable")[:, :9]
        assert np.array_equal(keys, want.astype(np.uint64)) and np.array_equal(scores, np.take_along_axis(full, want, 1))
        assert (counts == 9).all()
        thr = float(np.median(scores))
        _, s2, c2, _ = R.reference(base, q, 9, metric, drop=drop, threshold=thr, integer=True)
        assert np.array_equal(c2, (scores <= thr).sum(1))


CUT = 65536                        # rows of the cut the fixtures are checked on: every prefix and every "behind" position lies inside


def _cut(store, metric, cache={}):
    """the first CUT rows of the store's offset background.  (The background is drawn row-wise from one stream, and its distance
    from the planted rows is bounded by construction, not by the draw: what holds on the cut holds on the 262 144 rows.)"""
    if (store, metric) not in cache:
        if store == "D768":
            cache.clear()
        dim, f16 = R.STORES[store]
        cache[store, metric] = R.background("offset", metric, dim, f16, seed=1, rows=CUT)
    return cache[store, metric]


ALL_RUNS = [(c, l, None) for c, l in R.OFFSET_RUNS] + R.PREFIX_RUNS


@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
@pytest.mark.parametrize("case,layout,variant", ALL_RUNS)
def test_every_offset_fixture_meets_its_preconditions(case, layout, variant, metric):
    """every planted fixture of tests/test_gpu_seed_routes.py (the same builder, seed_ref.offset_fixture): values exact in the store's
    type, the fp64 top-k is the expected set, the runner-up is beyond twice the select band, and — the radius runs use cases 6 and
    11 on the spread layout — a radius between the near and the far rows clears every reference score by more than the band.

    Rank sensitivity: the k-th planted row stands alone, so the bound taken ONE RANK TOO LOW (the (k-1)-th of seed_bound_kernel's
    256 minima, or the (k-1)-th score of the prefix list seed_gtau_kernel reads) plus the slack lies BELOW the k-th planted score
    for every query: a kernel with that mistake drops the row and the query comes back short."""
    store = R.CASES[case][0]
    dim, f16 = R.STORES[store]
    base = _cut(store, metric)
    assert base.min() >= 1000 and base.max() < 1016
    fx = R.offset_fixture(case, metric, layout, variant, rows=CUT)
    pos, k, drop = fx["pos"], fx["k"], fx["drop"]
    what = "%s %s %s %s" % (case, metric, layout, variant)
    save = base[pos].copy()
    try:
        base[pos] = fx["planted"].astype(base.dtype)
        assert np.array_equal(base[pos].astype(np.float64), fx["planted"])           # exact in the store's element type
        q = fx["queries"].astype(base.dtype)
        assert np.array_equal(q.astype(np.float64), fx["queries"])
        keys, scores, counts, runner = R.reference(base, q, k, metric, drop=drop, planted=pos, integer=True)
        bn = float((base[fx["expect"]].astype(np.float64) ** 2).sum(1).max())
        _, band = R.bands(bn, q, metric)
        R.check_planted_fixture(keys, scores, counts, runner, fx["expect"], band, k, what=what)
        if fx["nfar"]:
            # one rank too low, on the prefix this case seeds from (unseeded controls: the same fixture, nothing to drop it)
            word = R.case_route(case, None if drop is None else int(R.ROWS * (~drop).mean()))
            prefix = R.SEED_ROWS256 if word & R.SCAN256 else R.SEED_ROWS
            s = R.scores64(base[:prefix], q, metric)
            if drop is not None:
                s[:, drop[:prefix]] = np.inf
            low = np.sort(s, 1)[:, k - 2]                                             # the prefix's true (k-1)-th score ...
            if word >> R.SEED_SHIFT & 3 == 1 and layout != "one_share":
                low = np.array([R.seed_bound_model(r, k - 1) for r in s])             # ... or the (k-1)-th of the 256 minima
            inside = np.isfinite(low)
            assert inside.all() or variant in ("wholly", "k-1")
            sl = R.slack_of(metric, q, bn, low)
            assert (low + sl < scores[:, k - 1])[inside].all(), "%s: a bound one rank too low still admits the k-th planted row" % what
            assert (scores[:, k - 1] - scores[:, k - 2] > 2 * band).all()
        if (case, layout, variant) in (("c06", "spread", None), ("c11", "spread", None)):
            thr = R.offset_radius(metric, fx["centre"], dim)
            _, s2, c2, _ = R.reference(base, q, k, metric, drop=drop, threshold=thr, integer=True)
            assert (c2 == k - 1).all()
            assert (np.abs(scores - thr) > band[:, None]).all()
    finally:
        base[pos] = save

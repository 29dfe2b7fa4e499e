"""Reference side of the seeded-bound route tests (tests/test_gpu_seed_routes.py, tests/test_seed_reference_cpu.py).

Three things, none of which calls the library:
  * a restatement of the dispatch of flat_scan_prepared / flat_scan_gather (zvec_amd/csrc/api_flat_scan.inc.h) that returns the route
    word zvec_hip_ctx_last_route must report for a shape;
  * a model of seed_bound_kernel's bound (k-th smallest of 256 strided minima);
  * the fixtures (stores, data kinds, planted layouts, filters), their fp64 reference and the preconditions the fixtures must meet.
"""
import numpy as np

# ---- route word (include/zvec_hip.h, zvec_hip_ctx_last_route) ------------------------------------------------------------------------
DENSE, NG1, NG2, NG4, M16, SCAN8, SCAN256, GATHER, COMPACT, EXCL = (1 << i for i in range(10))
SEED_SHIFT, PREFIX_SHIFT, SHAPE_MASK = 10, 16, 0x3ff
SEED_NONE, SEED_BOUND, SEED_GTAU = 0, 1 << SEED_SHIFT, 2 << SEED_SHIFT
_NAMES = ["dense", "ng1", "ng2", "ng4", "m16", "scan8", "scan256", "gather", "compact", "excl"]


def describe(word):
    shape = lambda w: "+".join(n for i, n in enumerate(_NAMES) if w >> i & 1) or "-"
    seed = {0: "none", 1: "seed_bound", 2: "seed_gtau"}.get(word >> SEED_SHIFT & 3, "?")
    return "main %s / %s / prefix %s (0x%x)" % (shape(word & SHAPE_MASK), seed, shape(word >> PREFIX_SHIFT & SHAPE_MASK), word)


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------
TILE_N, TILE_K, QGROUP, W8_ROWS, S256_ROWS = 128, 32, 32, 128, 256
SLAB = TILE_N * TILE_K
LDS_LIMIT = 160 * 1024
SEED_MIN_ROWS, SEED_ROWS, SEED_ROWS256 = 64 * 4096, 4096, 16384
CACHE_BYTES, SEED_DUMP_BYTES, DENSE_BYTES = 64 << 20, 256 << 20, 128 << 20


def scan_lds_bytes(ng, k, m16=False):
    rows = 32 if m16 else ng * QGROUP
    return (2 * rows * TILE_K + 2 * SLAB + 7 * rows + 4 + 2 * rows * k) * 4


def scan8_lds_bytes(k):
    return (2 * W8_ROWS * TILE_K + 2 * SLAB + 7 * W8_ROWS + 4 + 2 * W8_ROWS * k) * 4


def scan256_lds_bytes(k):
    return 2 * 64 * 1024 + 2048 + 7 * S256_ROWS * 4 + 2 * S256_ROWS * k * 4


def merge_fits(k):
    return k * 12 + 16 <= 60 * 1024


def pick_ng(rows_wanted, k):
    ng = 4
    while ng > 1 and (ng // 2) * QGROUP >= rows_wanted:
        ng //= 2
    while ng >= 1 and scan_lds_bytes(ng, k) > LDS_LIMIT - 1024:
        ng //= 2
    return ng


def padded_words(dim, f16, cosine=False):
    """4-byte words per stored row (StoreView::configure): fp32 rows pad to 32 floats, fp16 rows to 64 halves"""
    dscan = dim - ((2 if f16 else 1) if cosine else 0)
    return (dscan + 63) // 64 * 64 // 2 if f16 else (dscan + TILE_K - 1) // TILE_K * TILE_K


def route_word(rows, dpad, f16, queries, k, exclude=False, kept=None, user=True):
    """the route word of a flat search of `queries` queries for k over `rows` rows of `dpad` words (default options: scan256 = 1, no
    tuning knob); exclude: an exclude set is given, kept: rows it keeps.  user=False: the seeding prefix's own (internal) scan."""
    if rows == 0:
        return 0
    if exclude and user and rows >= 65536:
        can_gather = queries > 2 * QGROUP and pick_ng(queries, k) == 4 and scan8_lds_bytes(k) <= LDS_LIMIT - 1024
        if kept <= (0.9 if can_gather else 0.5) * rows:
            if kept == 0:
                return 0
            if can_gather:
                w = GATHER
                if kept >= 64 * SEED_ROWS and k <= 64 and merge_fits(k):
                    w |= SEED_GTAU | GATHER << PREFIX_SHIFT
                return w
            return COMPACT | route_word(kept, dpad, f16, queries, k, False, None, user)
    resident = rows * dpad * 4 <= CACHE_BYTES
    ntiles = (rows + TILE_N - 1) // TILE_N
    want_a = resident and not exclude and k > 8 and ntiles * TILE_N * 4 * queries <= DENSE_BYTES
    want_b = pick_ng(queries, k) < 1
    if want_b and not merge_fits(k):
        return 0                                            # (unsupported)
    if (want_a or want_b) and merge_fits(k):
        return DENSE | (EXCL if exclude else 0)
    can256 = f16 and not exclude and queries >= S256_ROWS and dpad // TILE_K >= 2 and scan256_lds_bytes(k) <= LDS_LIMIT \
        and queries * dpad * 4 < 1 << 32
    wide = not resident and pick_ng(queries, k) == 4 and queries > 2 * QGROUP and scan8_lds_bytes(k) <= LDS_LIMIT - 1024
    wide256 = wide and can256
    w = 0
    if rows >= SEED_MIN_ROWS and k <= 64 and queries >= 16:
        prefix = SEED_ROWS256 if wide256 else SEED_ROWS
        if not exclude and prefix * 4 * queries <= SEED_DUMP_BYTES:
            w |= SEED_BOUND
        else:
            w |= SEED_GTAU | (route_word(prefix, dpad, f16, queries, k, exclude, None, False) & SHAPE_MASK) << PREFIX_SHIFT
    ng = pick_ng(queries, k)
    if resident and ng > 1:
        ng = 1
    if wide256:
        w |= SCAN256
    elif wide:
        w |= SCAN8
    elif ng == 1 and queries <= 16:
        w |= M16
    else:
        w |= {1: NG1, 2: NG2, 4: NG4}[ng]
    return w | (EXCL if exclude else 0)


def prefix_rows(rows, dpad, f16, queries, k, exclude=False):
    """rows of the seeding prefix of that search (0: not seeded)"""
    w = route_word(rows, dpad, f16, queries, k, exclude, rows)
    if not w >> SEED_SHIFT & 3:
        return 0
    return SEED_ROWS256 if w & SCAN256 else SEED_ROWS


# ---- seed_bound_kernel ----------------------------------------------------------------------------------------------------------------
def seed_bound_model(row, k):
    """the unslacked bound seed_bound_kernel takes from one query's prefix scores: thread t of 256 keeps the minimum of the columns
    t, t + 256, ...; the k-th smallest of the 256 minima (+inf when fewer than k shares hold a finite score: no seeding)"""
    row = np.asarray(row, np.float64)
    pad = np.full((-len(row)) % 256, np.inf)
    mins = np.concatenate([row, pad]).reshape(-1, 256).min(0)
    return float(np.sort(mins)[k - 1]) if k <= 256 else float("inf")


# ---- stores, data kinds, layouts ------------------------------------------------------------------------------------------------------
ROWS = SEED_MIN_ROWS                                        # 262 144: the smallest seeded size
STORES = {                                                   # name -> (dim, fp16)
    "R32": (24, False),                                      # 32 words: 32 MiB, cache resident
    "S32": (72, False),                                      # 96 words: 96 MiB, streamed
    "S16": (136, True),                                      # 96 words: 96 MiB, three k-steps
    "D768": (768, False),                                    # 768 MiB, streamed
}
METRICS = {"SquaredEuclidean": 0, "InnerProduct": 1, "Cosine": 2}


def store_route(store, queries, k, exclude=False, kept=None):
    dim, f16 = STORES[store]
    return route_word(ROWS, padded_words(dim, f16), f16, queries, k, exclude, kept)


def layout_positions(layout, n, prefix=SEED_ROWS):
    """n planted positions inside the prefix (late: behind the first 4096 rows of a 16 384-row prefix)"""
    i = np.arange(n)
    if layout == "spread":                                   # distinct residues mod 256 (61 is odd), many tiles
        pos = 3 + 61 * i
    elif layout == "one_share":                              # one thread's share of seed_bound_kernel
        pos = 5 + 256 * i
    elif layout == "one_chunk":                              # one 128-row tile
        pos = 10 * TILE_N + 1 + 2 * i
    elif layout == "late":
        pos = SEED_ROWS + 5 + 183 * i
        prefix = SEED_ROWS256
    elif layout == "behind":                                 # outside every prefix
        pos = 3 * SEED_ROWS256 + 7 + 61 * i
        prefix = ROWS
    else:
        raise ValueError(layout)
    assert n <= 68 and pos.max() < prefix and len(set(pos.tolist())) == n, (layout, n)
    if layout == "spread":
        assert len(set((pos % 256).tolist())) == n
    if layout == "one_share":
        assert len(set((pos % 256).tolist())) == 1
    if layout == "one_chunk":
        assert len(set((pos // TILE_N).tolist())) == 1
    return pos


def background(kind, metric, dim, f16, seed, rows=ROWS):
    """the unplanted rows of a store.  offset: 1000 + integers, exact in fp32 and fp16 — L2 rows in [11, 16) around a centre in
    [0, 2), inner-product rows in [0, 8) under a centre in [12, 15), so that EVERY background row is further than 75 dim (L2) or
    4000 dim (inner product) behind the last planted row, whatever the draw; exact: integers in [-6, 6]; gaussian: unit normal."""
    rng = np.random.default_rng([seed, dim, METRICS[metric], ("offset", "exact", "gaussian").index(kind)])
    dt = np.float16 if f16 else np.float32
    if kind == "offset":
        lo, hi = (11, 16) if metric == "SquaredEuclidean" else (0, 8)
        base = rng.integers(lo, hi, (rows, dim), dtype=np.int16).astype(dt)
        base += dt(1000.0)
        return base
    if kind == "exact":
        return rng.integers(-6, 7, (rows, dim), dtype=np.int8).astype(dt)
    return rng.standard_normal((rows, dim), dtype=np.float32).astype(dt)


def offset_centre(metric, dim, seed):
    rng = np.random.default_rng([seed, dim, 77])
    lo, hi = (0, 2) if metric == "SquaredEuclidean" else (12, 15)
    return 1000.0 + rng.integers(lo, hi, dim).astype(np.float64)


def offset_planted(metric, centre, n, nfar):
    """n rows next to the centre: n - nfar NEAR rows and, last, nfar FAR rows (1, or 2 where a filter takes one of them out again), so
    that the k-th planted row stands alone: further above the (k - 1)-th than the seeding slack (a bound taken one rank too low
    drops it), more than twice the select band below the best background row, and a radius fits between the groups, further than
    the band from both.
    L2: near rows at distances 0, 1, 2 (row i: i % 3 coordinates raised by one: far below one ulp of the norms); a far row is the
    centre raised by five everywhere and by six in one place (distance ~25 dim: the slack is ~16.5 dim, the background beyond 100 dim).
    Inner product: near rows the centre with one coordinate raised (products within a few units of each other); a far row the centre
    with eight coordinates lowered by four (product ~32 000 lower: the slack is ~8.2 dim, every background row ~4000 dim lower)."""
    d = len(centre)
    rows = np.repeat(centre[None, :], n, 0)
    for i in range(n):
        near = i < n - nfar
        if metric == "SquaredEuclidean":
            if near:
                for t in range(i % 3):
                    rows[i, (i + 7 * t) % d] += 1.0
            else:
                rows[i] += 5.0
                rows[i, i % d] += 1.0
        elif near:
            rows[i, i % d] += 1.0
        else:
            rows[i, (i + np.arange(8)) % d] -= 4.0
    return rows


def offset_radius(metric, centre, dim):
    """a radius between the near and the far planted rows for every query of offset_queries"""
    if metric == "SquaredEuclidean":
        return 12.5 * dim
    return -float(centre @ centre) - 2026.0 + 16000.0


def offset_queries(metric, centre, nq):
    """the centre with one coordinate raised: by 1, 2 or 3 (L2), by 1 (inner product)"""
    d = len(centre)
    q = np.repeat(centre[None, :], nq, 0)
    i = np.arange(nq)
    q[i, i % d] += (1.0 + (i // d) % 3) if metric == "SquaredEuclidean" else 1.0
    return q


def drop_mask(share, seed, keep=(), drop=(), rows=ROWS):
    """exclude set: `share` of the rows at random, then `keep` kept and `drop` dropped whatever the draw"""
    rng = np.random.default_rng([seed, int(share * 1000)])
    m = rng.random(rows) < share
    m[np.asarray(keep, np.int64)] = False
    m[np.asarray(drop, np.int64)] = True
    return m


# ---- fp64 reference -------------------------------------------------------------------------------------------------------------------
def reference(base, q, k, metric, drop=None, threshold=None, planted=None, integer=False, chunk=16384):
    """Flat search in fp64, chunked over the rows.  L2 |q|^2 + |b|^2 - 2 q.b, inner product -q.b, cosine 1 - q.b over the first
    d columns (rows and queries already transformed), every term in fp64: exact on the integer kinds, and on gaussian rows within
    2^-52 (|q|^2 + |b|^2) d of the direct sum — eight orders below the bands it is compared with.  Excluded positions are removed,
    the k best taken by (score, position) — `integer`: through the exact key score * rows + position —, the radius applied to the
    score rounded to fp32 (what the search reports).  Returns keys [nq][k] (positions), scores, counts, and `runner`: the best
    score outside `planted` per query (None without)."""
    m = METRICS[metric]
    n, nq = base.shape[0], q.shape[0]
    d = base.shape[1] - (1 if m == 2 else 0)
    q64 = np.asarray(q, np.float64)[:, :d]
    qn = (q64 ** 2).sum(1)
    best_s = np.full((nq, 0), np.inf)
    best_p = np.zeros((nq, 0), np.int64)
    runner = np.full(nq, np.inf)
    pl = np.zeros(n, bool)
    if planted is not None:
        pl[np.asarray(planted, np.int64)] = True
    for o in range(0, n, chunk):
        b = np.asarray(base[o:o + chunk], np.float64)[:, :d]
        dot = q64 @ b.T
        s = qn[:, None] + (b ** 2).sum(1)[None, :] - 2.0 * dot if m == 0 else (-dot if m == 1 else 1.0 - dot)
        if drop is not None:
            s[:, drop[o:o + chunk]] = np.inf
        if planted is not None:
            rest = np.where(pl[None, o:o + chunk], np.inf, s)
            runner = np.minimum(runner, rest.min(1))
        pos = np.arange(o, o + b.shape[0])
        kk = min(k, b.shape[0])
        key = s * float(n) + pos[None, :] if integer else s
        part = np.argpartition(key, kk - 1, axis=1)[:, :kk]
        best_s = np.concatenate([best_s, np.take_along_axis(s, part, 1)], 1)
        best_p = np.concatenate([best_p, pos[part]], 1)
    order = np.lexsort((best_p, best_s), axis=1)[:, :k]
    scores = np.take_along_axis(best_s, order, 1)
    keys = np.take_along_axis(best_p, order, 1)
    ok = np.isfinite(scores)
    if threshold is not None:
        ok &= ~(scores.astype(np.float32) > np.float32(threshold))
    counts = ok.sum(1).astype(np.uint32)
    assert all(ok[i, :counts[i]].all() for i in range(nq))          # (ascending scores: what is cut is the tail)
    return keys.astype(np.uint64), scores, counts, (runner if planted is not None else None)


def bands(base_norm_max, q, metric, cosine_dim=None):
    """L2 reported score within 2e-6 score + 1e-6, ids free inside 4e-6 (|q|^2 + |b|^2); inner product and cosine
    within 4e-6 |q||b|.  Returns the keyword arguments of tie_tolerant_compare and the per-query select band."""
    q64 = np.asarray(q, np.float64)
    if cosine_dim is not None:
        q64 = q64[:, :cosine_dim]
    qn = (q64 ** 2).sum(1)
    if metric == "SquaredEuclidean":
        band = 4e-6 * (qn + base_norm_max)
        return dict(rtol=2e-6, atol=1e-6, select_band=band), band
    band = 4e-6 * np.sqrt(qn * base_norm_max)
    return dict(rtol=4e-6, scale=np.sqrt(qn * base_norm_max)), band


def check_planted_fixture(ref_keys, ref_scores, ref_counts, runner, expect, band, k, what=""):
    """the preconditions of a planted fixture: the fp64 reference returns exactly the expected rows for every query, and the best
    other row is more than twice the select band behind the k-th"""
    want = set(int(p) for p in expect)
    assert len(want) == k, "%s: %d planted rows for k = %d" % (what, len(want), k)
    for i in range(len(ref_counts)):
        assert int(ref_counts[i]) == k and set(ref_keys[i].tolist()) == want, "%s query %d: fp64 top-k is not the planted set" % (what, i)
        gap = runner[i] - ref_scores[i, k - 1]
        assert gap > 2.0 * band[i], "%s query %d: runner-up gap %r within twice the band %r" % (what, i, gap, band[i])


# ---- the case table: (store, queries, k, share dropped) -> the route word spelled out ------------------------------------------------
def _gtau(prefix):
    return SEED_GTAU | prefix << PREFIX_SHIFT


CASES = {
    "c01": ("R32", 16, 8, 0.0, M16 | SEED_BOUND),
    "c02": ("R32", 17, 1, 0.0, NG1 | SEED_BOUND),
    "c03": ("R32", 64, 9, 0.0, DENSE),                                        # control: the dense-score path is not seeded
    "c04": ("S32", 16, 64, 0.0, M16 | SEED_BOUND),                            # the largest seeded k
    "c05": ("S32", 40, 10, 0.0, NG2 | SEED_BOUND),
    "c06": ("S32", 65, 10, 0.0, SCAN8 | SEED_BOUND),
    "c07a": ("S32", 65, 65, 0.0, SCAN8),                                      # controls: one step past k = 64 ...
    "c07b": ("S32", 15, 10, 0.0, M16),                                        # ... and one below 16 queries
    "c08": ("S16", 256, 10, 0.0, SCAN256 | SEED_BOUND),                       # 16 384-row prefix
    "c09": ("S16", 255, 10, 0.0, SCAN8 | SEED_BOUND),
    "c10": ("S16", 4097, 10, 0.0, SCAN256 | _gtau(NG1)),                      # the prefix dump would pass 256 MiB
    "c11": ("S32", 65, 10, 0.05, SCAN8 | EXCL | _gtau(NG1 | EXCL)),
    "c12": ("S32", 40, 10, 0.4, NG2 | EXCL | _gtau(NG1 | EXCL)),
    "c15a": ("D768", 65, 10, 0.0, SCAN8 | SEED_BOUND),
    "c15b": ("D768", 65, 10, 0.05, SCAN8 | EXCL | _gtau(NG1 | EXCL)),
}


def case_route(name, kept=None):
    store, nq, k, share, _ = CASES[name]
    if kept is None:
        kept = int(round(ROWS * (1.0 - share)))
    return store_route(store, nq, k, share > 0, kept)


# ---- the planted (offset) fixtures of the GPU tests, one definition for both sides ---------------------------------------------------
# (case, layout): every case on the spread layout; the share layout where seed_bound_kernel seeds a k > 1; the late layout in front of
# the 16 384-row prefix; one chunk wherever the prefix is a scan with lists (its single full list publishes exactly the k-th score)
OFFSET_RUNS = [("c01", "spread"), ("c02", "spread"), ("c03", "spread"), ("c04", "spread"), ("c05", "spread"), ("c05", "one_share"),
               ("c06", "spread"), ("c06", "one_share"), ("c07a", "spread"), ("c07b", "spread"), ("c08", "spread"), ("c08", "late"),
               ("c09", "spread"), ("c10", "spread"), ("c10", "one_chunk"), ("c11", "spread"), ("c11", "one_chunk"), ("c12", "spread"),
               ("c12", "one_chunk"), ("c15a", "spread"), ("c15a", "one_chunk"), ("c15b", "spread"), ("c15b", "one_chunk")]
PREFIX_VARIANTS = ["wholly", "k-1", "k"]                      # case 13, on case 11's shape
PREFIX_RUNS = [("c11", layout, v) for layout in ("spread", "one_chunk") for v in PREFIX_VARIANTS]
QUERY_POOL = 64                                               # batches beyond 256 queries repeat this many distinct ones


def offset_fixture(case, metric, layout, variant=None, rows=ROWS):
    """One planted fixture: dict(pos, planted, drop, expect, queries, qmap, k, nfar).  Unfiltered cases plant k rows (k - 1 near,
    one far; k = 1: one near row).  Filtered cases plant k + 3 (k + 1 near, two far) and exclude planted rows 0, 2 and the last: two
    of the nearest and one far row must not come back, and k - 1 near rows + one far row remain.  variant (case 13): the prefix is
    excluded but for the kept planted rows, of which `wholly` puts all behind the prefix, `k-1` the far one, `k` none."""
    store, nq, k, share, _ = CASES[case]
    dim, _f16 = STORES[store]
    centre = offset_centre(metric, dim, seed=1)
    filtered = share > 0
    n, nfar = (k + 3, 2) if filtered else (k, 1 if k > 1 else 0)
    pos = layout_positions(layout, n)
    gone = np.asarray([0, 2, n - 1]) if filtered else np.zeros(0, np.int64)
    behind = layout_positions("behind", n)
    if variant == "wholly":
        pos = behind
    elif variant == "k-1":
        pos = pos.copy()
        pos[n - 2] = behind[n - 2]                            # the far row that stays
    drop = None
    if filtered:
        drop = drop_mask(share, seed=3, keep=pos, drop=pos[gone], rows=rows)
        if variant is not None:
            drop[:SEED_ROWS] = True
            drop[pos] = False
            drop[pos[gone]] = True
    uniq = min(nq, 256 if nq <= 256 else QUERY_POOL)
    return dict(pos=pos, planted=offset_planted(metric, centre, n, nfar), drop=drop, expect=np.setdiff1d(pos, pos[gone]),
                queries=offset_queries(metric, centre, uniq), qmap=np.arange(nq) % uniq, k=k, nfar=nfar, centre=centre)


def slack_of(metric, q, rows_norm_max, kth):
    """the seeding kernels' slack for queries q ([nq][d], fp64): 8e-6 mag + 1e-6 |k-th|, mag from |q|^2 and the largest |b|^2 of
    the k rows that carry the bound"""
    qn = (np.asarray(q, np.float64) ** 2).sum(1)
    mag = qn + rows_norm_max if metric == "SquaredEuclidean" else np.sqrt(qn * rows_norm_max)
    return 8e-6 * mag + 1e-6 * np.abs(kth)


def scores64(rows, q, metric):
    """fp64 scores [nq][rows] (L2 by the expansion, inner product -q.b): exact on integer data"""
    b, q64 = np.asarray(rows, np.float64), np.asarray(q, np.float64)
    dot = q64 @ b.T
    return (q64 ** 2).sum(1)[:, None] + (b ** 2).sum(1)[None, :] - 2.0 * dot if metric == "SquaredEuclidean" else -dot

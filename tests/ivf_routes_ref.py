"""Fixtures and fp64 reference of the IVF route tests (tests/test_gpu_ivf_routes.py, tests/test_ivf_routes_reference_cpu.py): every
route of ivf_search_core from GIVEN probe lists (zvec_hip_ivf_search_probes_dev), every metric, both element types, the dims around
the scan's k-step.  numpy only; nothing here touches the GPU or the library.  The probe rule, the plan, the bitset packing and the
route rule are those of tests/ivf_plan_ref.py.

  index      24 lists (SIZES: 0, 1, 127, 128, 129 rows, four lists of 400 - 600, small ones; 2818 rows).  The two largest hold 1020
             rows — one run of the direct selection at nprobe 2 —, the five largest 1959 — two runs at nprobe 5.
  dims       a k-step of the scan is 128 bytes of a stored row: 32 floats, 64 halves (TILE_K words, api_types.inc.h).  Per element
             type one dim below it, one exactly it, one a little above, one of several k-steps and a remainder.  Cosine rows carry
             the norm on top (d + 1 floats, d + 2 halves).  fp32 dim 32 under L2 / inner product is a whole k-step without padding:
             the raw_rows condition of api_ivf_core.inc.h.
  probes     [nq][nprobe] list ids, distinct within a query, in no order (a random permutation; one of the four large lists is put
             among the counted entries so that every query has a few hundred candidates); probe_cnt[q] = nprobe - q % nprobe.
  kinds      exact: integers in [0, 8), six rows in ten drawn from a pool of 40 points — every L2 / inner-product score is exact in
             fp32 and fp16 and the k-th place is tied in most queries, inside one list and across lists;  gaussian: unit normal,
             rounded to binary16 for fp16 indexes (the reference works on the widened values).  Cosine: gaussian only.
  reference  fp64 scores (squared L2, minus inner product, 1 - ip over the normalised part); candidates = the probed prefix by
             ivf_plan_ref.probe_rule over the given ranks and counts, minus the excluded positions, minus the rows beyond the
             radius; order (score, probe rank, place in list).  `wrong` makes it wrong in one way (WRONG): the CPU test shows that
             every such mistake changes the answer of every cell."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_plan_ref as P  # noqa: E402
import seed_ref as S  # noqa: E402

L2, IP, COS = "SquaredEuclidean", "InnerProduct", "Cosine"
METRICS = (L2, IP, COS)
DTYPES = ("fp32", "fp16")
KSTEP = {"fp32": 32, "fp16": 64}                            # elements of one 128-byte k-step
DIMS = {"fp32": (5, 32, 36, 130), "fp16": (6, 64, 68, 200)}
NORM_SLOTS = {"fp32": 1, "fp16": 2}                         # cosine: the fp32 norm behind the d normalised values
RAW_ROWS = ("fp32", 32)                                     # dim_in == dscan == dpad, row_bytes == dpad x 4 (not under cosine)
NP_DTYPE = {"fp32": np.float32, "fp16": np.float16}

SIZES = np.asarray([17, 600, 0, 127, 33, 420, 1, 128, 64, 410, 129, 5, 400, 90, 40, 70, 12, 3, 50, 25, 8, 2, 100, 84], np.int64)
NLIST = SIZES.size
LARGE = (1, 5, 9, 12)                                       # the lists of 400 rows and more
NO_LIMIT = 0xffffffff

# route cell -> (name, nprobe, ((nq, k), (nq, k))): both batch sizes of the issue on each, k as the route needs
ROUTES = {
    "block_topk": (P.ROUTE_DIRECT_BLOCK_TOPK, 5, ((1, 10), (8, 64))),
    "select_two_step": (P.ROUTE_DIRECT_SELECT, 5, ((1, 100), (8, 65))),
    "select_one_step": (P.ROUTE_DIRECT_SELECT, 2, ((1, 10), (8, 100))),
    "tile": (P.ROUTE_TILE, 6, ((9, 10), (40, 100))),
    "large_k": (P.ROUTE_LARGE_K, 8, ((9, 500), (40, 500))),
}
DIRECT = ("block_topk", "select_two_step", "select_one_step")
VARIANTS = ("plain", "exclusion", "radius", "radius_far", "max_scan")
WRONG = ("last_kstep", "probe_cnt", "sorted_lists", "exclusion", "radius", "radius_sign")


def kinds_of(metric):
    return ("gaussian",) if metric == COS else ("exact", "gaussian")


def runs_of(nprobe):
    """runs of 1024 candidates of the direct selection (api_ivf_core.inc.h: stride, runs)"""
    rows = int(np.sort(SIZES)[::-1][:nprobe].sum())
    stride = (max(rows, 1) + 63) // 64 * 64
    return (stride + P.RUN - 1) // P.RUN


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def cosine_rows(x, dtype):
    """rows of d values -> normalised rows with the fp32 norm behind them: d + 1 floats, or d halves + the norm's four bytes in
    two half slots (what the reference's cosine converter stores)"""
    x = np.asarray(x, np.float32)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    unit = (x / norm[:, None]).astype(np.float32)
    if dtype == "fp32":
        return np.concatenate([unit, norm[:, None]], 1)
    out = np.zeros((x.shape[0], x.shape[1] + 2), np.float16)
    out[:, :-2] = unit.astype(np.float16)
    out.view(np.uint16)[:, -2:] = np.ascontiguousarray(norm[:, None]).view(np.uint16)
    return out


def _draw(kind, n, d, rng, pool=None):
    if kind == "gaussian":
        return rng.standard_normal((n, d)).astype(np.float32)
    x = rng.integers(0, 8, (n, d)).astype(np.float32)
    if pool is not None:
        planted = rng.random(n) < 0.6
        x[planted] = pool[rng.integers(0, len(pool), int(planted.sum()))]
    return x


def index(metric, dtype, d, kind):
    """one index: dict(dim (at the ABI), d (scanned), vecs, cent, sizes, ...); vecs / queries in the stored element type"""
    assert kind in kinds_of(metric)
    rng = np.random.default_rng([d, DTYPES.index(dtype), METRICS.index(metric), kind == "gaussian"])
    n = int(SIZES.sum())
    pool = rng.integers(0, 8, (40, d)).astype(np.float32)
    x = _draw(kind, n, d, rng, pool)
    vecs = cosine_rows(x, dtype) if metric == COS else x.astype(NP_DTYPE[dtype])
    dim = vecs.shape[1]
    cent = np.zeros((NLIST, dim), NP_DTYPE[dtype])            # (never ranked: every search here is given its probe lists)
    cent[:, 0] = 1.0
    return dict(name="%s %s d%d %s" % (metric, dtype, d, kind), metric=metric, dtype=dtype, d=d, dim=dim, kind=kind, sizes=SIZES,
                nlist=NLIST, vecs=vecs, cent=cent, seed=[d, DTYPES.index(dtype), METRICS.index(metric)])


def queries(ix, nq):
    rng = np.random.default_rng(ix["seed"] + [nq, 77])
    x = _draw(ix["kind"], nq, ix["d"], rng)
    return cosine_rows(x, ix["dtype"]) if ix["metric"] == COS else x.astype(NP_DTYPE[ix["dtype"]])


def probe_lists(nq, nprobe, seed):
    """ids [nq][nprobe] (a random permutation each: distinct, in no order) and counts [nq] in 1 ... nprobe; one large list stands
    among the counted entries of every query"""
    rng = np.random.default_rng([seed, nq, nprobe])
    ids = np.zeros((nq, nprobe), np.int64)
    cnt = np.asarray([nprobe - q % nprobe for q in range(nq)], np.int64)
    for q in range(nq):
        row = rng.permutation(NLIST)[:nprobe]
        big = LARGE[q % len(LARGE)]
        at = q % int(cnt[q])
        if big in row[:cnt[q]]:
            pass
        elif big in row:
            j = int(np.nonzero(row == big)[0][0])
            row[at], row[j] = row[j], row[at]
        else:
            row[at] = big
        ids[q] = row
    return ids, cnt


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
def scores64(metric, rows, q, d, drop_from=None):
    """fp64 scores of one query over rows (stored values widened); drop_from: the dims from there on count for nothing"""
    b, v = np.asarray(rows, np.float64)[:, :d], np.asarray(q, np.float64)[:d]
    if drop_from is not None:
        b, v = b[:, :drop_from], v[:drop_from]
    if metric == L2:
        return ((b - v[None, :]) ** 2).sum(1)
    dot = b @ v
    return -dot if metric == IP else 1.0 - dot


def last_kstep(dtype, d):
    """first dim of the last k-step of the scan, whole or partial"""
    ks = KSTEP[dtype]
    return ((d + ks - 1) // ks - 1) * ks


def answer(ix, q, ids, cnt, k, max_scan=NO_LIMIT, excluded=None, radius=None, wrong=None):
    """the reference of one search.  Returns dict(pos [nq][k] list-order positions (-1 beyond the count), scores fp64, counts,
    probed (lists per query), scanned, gap (the (k+1)-th admitted score minus the k-th; inf where there is none), cand (all admitted
    scores, ascending))."""
    offs = P.list_offsets(ix["sizes"])
    nq = len(q)
    metric, d = ix["metric"], ix["d"]
    out = dict(pos=np.full((nq, k), -1, np.int64), scores=np.zeros((nq, k)), counts=np.zeros(nq, np.int64), probed=[],
               scanned=np.zeros(nq, np.int64), gap=np.full(nq, np.inf), cand=[])
    for i in range(nq):
        ranks = np.sort(ids[i]) if wrong == "sorted_lists" else np.asarray(ids[i], np.int64)
        ranks = ranks[:ids.shape[1] if wrong == "probe_cnt" else cnt[i]]
        pr, sc = P.probe_rule(ranks, ix["sizes"], max_scan)
        out["probed"].append(pr)
        out["scanned"][i] = sc
        cand = np.concatenate([np.arange(offs[l], offs[l + 1]) for l in pr] + [np.zeros(0, np.int64)]).astype(np.int64)
        if excluded is not None and wrong != "exclusion":
            cand = cand[~excluded[cand]]
        s = scores64(metric, ix["vecs"][cand], q[i], d, last_kstep(ix["dtype"], d) if wrong == "last_kstep" else None)
        if radius is not None and wrong != "radius":
            # (the search compares the fp32 score it reports; every radius here keeps its distance from every score)
            keep = ~(-s > radius) if wrong == "radius_sign" else ~(s > radius)
            cand, s = cand[keep], s[keep]
        order = np.argsort(s, kind="stable")
        best = order[:k]
        out["counts"][i] = best.size
        out["pos"][i, :best.size], out["scores"][i, :best.size] = cand[best], s[best]
        if order.size > k:
            out["gap"][i] = s[order[k]] - s[order[k - 1]]
        out["cand"].append(s[order])
    return out


def all_scores(ix, q, ids, cnt):
    """the scores of every row of every counted list, per query (no exclusion, no scan limit): what a radius must keep clear of"""
    offs = P.list_offsets(ix["sizes"])
    out = []
    for i in range(len(q)):
        cand = np.concatenate([np.arange(offs[l], offs[l + 1]) for l in ids[i, :cnt[i]]]).astype(np.int64)
        out.append(scores64(ix["metric"], ix["vecs"][cand], q[i], ix["d"]))
    return out


def norm_max(ix):
    return float((np.asarray(ix["vecs"], np.float64)[:, :ix["d"]] ** 2).sum(1).max())


def select_band(ix, q, bn=None):
    """per query the band of DESIGN §4 inside which the id set may differ (seed_ref.bands), with |b|^2 the index's largest"""
    bn = norm_max(ix) if bn is None else bn
    return S.bands(bn, np.asarray(q, np.float64)[:, :ix["d"]], ix["metric"])


def radius_between(ix, q, ids, cnt, k, plain):
    """a radius in the middle between two neighbouring scores that lie more than four bands apart (exact kinds: any two different
    scores), taken over the scores of every counted row of every query.  Of those gaps: the one that cuts the lists of as near to
    half of the queries as can be (a query is cut when its last reference score lies beyond the radius); one query alone: the gap
    nearest to the middle of its list"""
    last = np.asarray([plain["scores"][i, max(int(plain["counts"][i]) - 1, 0)] for i in range(len(q))])
    pool = np.unique(np.concatenate(all_scores(ix, q, ids, cnt)))
    band = 0.0 if ix["kind"] == "exact" else float(select_band(ix, q)[1].max())
    gaps = np.diff(pool)
    ok = np.nonzero(gaps > 4.0 * band)[0]
    mid = (pool[ok] + pool[ok + 1]) / 2.0
    if len(q) == 1:
        r = float(mid[np.argmin(np.abs(mid - plain["scores"][0, int(plain["counts"][0]) // 2]))])
    else:
        short = (last[None, :] > mid[:, None]).sum(1)
        r = float(mid[np.argmin(np.abs(short - len(q) / 2.0))])
    return float(np.float32(r))                              # (what the entry point takes)


def radius_far(ix, q, ids, cnt):
    return float(np.float32(max(float(s.max()) for s in all_scores(ix, q, ids, cnt)) + 1.0e6))


def exclusion_with_a_whole_list(ids, cnt, seed=5):
    """about 30 % of the positions, and every row of a large list that query 0 probes"""
    ex = P.exclusion(int(SIZES.sum()), seed)
    offs = P.list_offsets(SIZES)
    whole = [int(l) for l in ids[0, :cnt[0]] if l in LARGE][0]
    ex[offs[whole]:offs[whole + 1]] = True
    return ex, whole


def max_scan_that_cuts(ids, cnt):
    """a scan limit that ends the probe walk of some queries before their last counted list: the median of the rows the queries hold
    in front of it"""
    before = np.asarray([int(SIZES[ids[i, :cnt[i] - 1]].sum()) for i in range(len(cnt))], np.int64)
    return max(1, int(np.median(before[before > 0])))


def case(ix, route, batch):
    """everything one batch of one cell searches: queries, probe lists and the arguments of its five variants"""
    _, nprobe, batches = ROUTES[route]
    nq, k = batches[batch]
    q = queries(ix, nq)
    ids, cnt = probe_lists(nq, nprobe, 31 + batch)
    plain = answer(ix, q, ids, cnt, k)
    ex, whole = exclusion_with_a_whole_list(ids, cnt)
    variants = {
        "plain": dict(),
        "exclusion": dict(excluded=ex),
        "radius": dict(radius=radius_between(ix, q, ids, cnt, k, plain)),
        "radius_far": dict(radius=radius_far(ix, q, ids, cnt)),
        "max_scan": dict(max_scan=max_scan_that_cuts(ids, cnt)),
    }
    return dict(nq=nq, k=k, nprobe=nprobe, q=q, ids=ids, cnt=cnt, variants=variants, whole=whole, plain=plain)


def same(a, b):
    """equal counts and equal score lists (the rows may differ among equal scores)"""
    return np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["scores"], b["scores"])


# ---- the coarse pass alone: centroids whose ranking is untied by construction ----------------------------------------------------------
COARSE_NLIST, COARSE_STEP = 12, 0.25


def coarse_fixture(metric, dtype, nq, nlist=COARSE_NLIST, dim=8, step=COARSE_STEP):
    """centroids, queries (stored element type; cosine: with the norm slots) and the scanned dims.
    L2: the line of ivf_plan_ref (centroid l at x = 2 l, queries at x = 2 j + 0.5: distances |2 (j - l) + 0.5|, all different);
    inner product: centroid l = (l + 1) e0, queries with x0 = +-1, +-2, +-3 (scores -x0 (l + 1): a unit apart at least);
    cosine: unit centroids at the angles l x step in a plane, unit queries at j x step + step / 4 in that plane
    (1 - cos of |step (l - j) - step / 4|, all different, below pi)."""
    rng = np.random.default_rng([nq, nlist, METRICS.index(metric)])
    j = np.arange(nq) % nlist
    if metric == L2:
        cent, q = P.line_centroids(nlist, dim), P.line_queries(j, dim, rng)
    elif metric == IP:
        cent = np.zeros((nlist, dim), np.float32)
        cent[:, 0] = 1.0 + np.arange(nlist)
        q = rng.integers(0, 8, (nq, dim)).astype(np.float32)
        q[:, 0] = (1.0 + np.arange(nq) % 3) * np.where(np.arange(nq) % 2 == 0, 1.0, -1.0)
    else:
        assert step * nlist < np.pi
        th, ph = step * np.arange(nlist), step * j + step / 4.0
        cent, q = np.zeros((nlist, dim), np.float32), np.zeros((nq, dim), np.float32)
        cent[:, 0], cent[:, 1], q[:, 0], q[:, 1] = np.cos(th), np.sin(th), np.cos(ph), np.sin(ph)
        cent, q = cosine_rows(cent, dtype), cosine_rows(q, dtype)
    return cent.astype(NP_DTYPE[dtype]) if metric != COS else cent, q.astype(NP_DTYPE[dtype]) if metric != COS else q, dim


def coarse_ranking(metric, cent, q, d):
    """[nq][nlist] list ids by fp64 score of the stored values, and the sorted scores"""
    s = np.stack([scores64(metric, cent, q[i], d) for i in range(len(q))])
    order = np.argsort(s, axis=1, kind="stable")
    return order, np.take_along_axis(s, order, 1)

"""Model and fixtures of the HNSW graph build (zvec_hip_hnsw_build, DESIGN §3c "Building").

build_model is the insertion rule in fp64 numpy: rounds of nodes that search the graph as it stood when the round began, selection
by update_neighbors, reverse links by reverse_update_neighbors applied per (level, target) in ascending source id.  The kernels are
compared with it array for array.  levels_model is the integer level generator.  The fixtures are the shapes at which the rule takes
each of its paths; tests/test_hnsw_build_reference_cpu.py asserts from the model's own bookkeeping that they do."""
import bisect
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_ref as H  # noqa: E402

MAX_LEVEL = 15                      # HNSW_BUILD_MAX_LEVEL
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1

Params = collections.namedtuple("Params", "m m0 ef_construction prune_cnt min_neighbors scaling_factor")
Counters = collections.namedtuple("Counters", "rounds dists requests prunes")
Fixture = collections.namedtuple("Fixture", "rows params levels round_div round_max metric")


def params(m=50, m0=None, ef_construction=500, prune_cnt=None, min_neighbors=0, scaling_factor=None):
    """the defaults of the reference's builder (hnsw_builder.cc): m0 = 2m, prune_cnt = m, scaling_factor = m"""
    return Params(m, 2 * m if m0 is None else m0, ef_construction, m if prune_cnt is None else prune_cnt, min_neighbors,
                  m if scaling_factor is None else scaling_factor)


# ---- levels ----------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    """the output of the SplitMix64 generator whose state before the call is x"""
    z = (x + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def level_thresholds(sf):
    """thr[k-1]: r * sf^k < 2^53  <=>  r < thr[k-1], for k = 1 .. MAX_LEVEL"""
    return [-((-(1 << 53)) // sf ** k) for k in range(1, MAX_LEVEL + 1)]


def levels_model(n, sf, seed=0):
    """level of node i = the number of k >= 1 with (splitmix64(seed + i * GOLD) >> 11) * sf^k < 2^53, at most MAX_LEVEL"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + np.arange(n, dtype=np.uint64) * np.uint64(GOLD) + np.uint64(GOLD)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        r = (z ^ (z >> np.uint64(31))) >> np.uint64(11)
    out = np.zeros(n, np.uint32)
    for t in level_thresholds(int(sf)):
        out += (r < np.uint64(t)).astype(np.uint32)
    return out


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def rounds_of(levels, round_div, round_max):
    """[(first, end, entry point, top level)] of every round after the seed node 0"""
    n = len(levels)
    out = []
    s, entry, top = 1, 0, int(levels[0]) if n else 0
    while s < n:
        if levels[s] > top:
            out.append((s, s + 1, entry, top))
            entry, top = s, int(levels[s])
            s += 1
            continue
        size = 1 if round_div == 0 else min(max(s // round_div, 1), round_max)
        e = min(s + size, n)
        for j in range(s + 1, e):
            if levels[j] > top:
                e = j
                break
        out.append((s, e, entry, top))
        s = e
    return out


def distance_matrix(rows, metric):
    r = np.asarray(rows, np.float64)
    n = r.shape[0]
    if metric == "ip":
        return -(r @ r.T) + 0.0
    D = np.zeros((n, n))
    for i0 in range(0, n, 256):
        d = r[i0:i0 + 256, None, :] - r[None, :, :]
        D[i0:i0 + 256] = np.einsum("ijk,ijk->ij", d, d)
    return D


def keep_rule(W, D, cap, counter=None):
    """walk W (ascending (distance, id)) and keep c unless some kept s has d(c, s) <= d(c, base); stop at cap.
    counter[0] grows by the kept ids every candidate is compared with."""
    kept = []
    for d, c in W:
        if counter is not None:
            counter[0] += len(kept)
        if all(D[c, s] > d for s in kept):
            kept.append(c)
            if len(kept) >= cap:
                break
    return kept


def search_level(D, lists, i, ep, ef, stat):
    """step 3 of DESIGN §3c on one level's lists for the row of node i: no exclude bits, no scan limit, no threshold"""
    visited = {ep}
    R = [(D[i, ep], ep)]
    C = [(D[i, ep], ep)]
    while C:
        dc, c = C[0]
        if len(R) == ef and dc > R[-1][0]:
            break
        C.pop(0)
        coll = []
        for v in lists[c]:
            if v not in visited:
                visited.add(v)
                coll.append(v)
        stat[0] += len(coll)
        for v in coll:
            dv = D[i, v]
            if len(R) < ef or dv < R[-1][0]:
                bisect.insort(C, (dv, v))
                bisect.insort(R, (dv, v))
                if len(R) > ef:
                    R.pop()
    return R


def build_model(rows, p, levels=None, round_div=16, round_max=4096, metric="l2", seed=0, keys=None, book=None):
    """Returns (hnsw_ref.Graph or None for no rows, Counters).  book: a dict that receives what the fixtures must show —
    most requests one (level, target) received in one round, prunes that dropped a link the target had before, selections that
    took the shortcut, selections filled up to min_neighbors, rounds a node made of its own because it raised the top level."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    bk = dict(max_requests=0, max_requests_cap=0, dropped_links=0, shortcuts=0, selections=0, filled=0, own_rounds=0, round_sizes=[])
    if book is not None:
        book.update(bk)
        bk = book
    if n == 0:
        return None, Counters(0, 0, 0, 0)
    levels = levels_model(n, p.scaling_factor, seed) if levels is None else np.asarray(levels, np.uint32)
    D = distance_matrix(rows, metric)
    nlev = int(levels.max()) + 1
    lists = [[[] for _ in range(n)] for _ in range(nlev)]
    dists = [0]
    requests = prunes = 0
    plan = rounds_of(levels, round_div, round_max)
    entry, top = 0, int(levels[0])
    for s, e, entry, top in plan:
        bk["round_sizes"].append(e - s)
        if levels[s] > top:
            bk["own_rounds"] += 1
        reqs = []
        own = []
        for i in range(s, e):
            li = int(levels[i])
            ep = entry
            cur = D[i, ep]
            dists[0] += 1
            for level in range(top, li, -1):
                while True:
                    ids = lists[level][ep]
                    if not ids:
                        break
                    dists[0] += len(ids)
                    moved = False
                    for v in ids:
                        if D[i, v] < cur:
                            ep, cur, moved = v, D[i, v], True
                    if not moved:
                        break
            for level in range(min(li, top), -1, -1):
                cap = p.m0 if level == 0 else p.m
                W = search_level(D, lists[level], i, ep, p.ef_construction, dists)
                ep = W[0][1]
                bk["selections"] += 1
                if len(W) <= min(p.prune_cnt, cap):
                    sel = [v for _, v in W]
                    bk["shortcuts"] += 1
                else:
                    sel = keep_rule(W, D, cap, dists)
                    if len(sel) < p.min_neighbors:
                        bk["filled"] += 1
                        for _, v in W:
                            if len(sel) >= p.min_neighbors:
                                break
                            if v not in sel:
                                sel.append(v)
                own.append((level, i, sel))
                reqs.extend((level, t, i) for t in sel)
        for level, i, sel in own:                        # (nobody reads a new node's lists during its round)
            lists[level][i] = list(sel)
        requests += len(reqs)
        per_target = collections.Counter((l, t) for l, t, _ in reqs)
        for (l, t), c in per_target.items():
            cap = p.m0 if l == 0 else p.m
            if c > bk["max_requests"]:
                bk["max_requests"], bk["max_requests_cap"] = c, cap
        for level, t, i in sorted(reqs):
            cap = p.m0 if level == 0 else p.m
            lst = lists[level][t]
            if len(lst) < cap:
                lst.append(i)
                continue
            prunes += 1
            kept = keep_rule(sorted((D[t, x], x) for x in lst + [i]), D, cap)
            if any(x not in kept for x in lst):
                bk["dropped_links"] += 1
            lists[level][t] = kept
    if plan:
        s, e, entry, top = plan[-1]
        if levels[s] > top:
            entry, top = s, int(levels[s])
    upper = {i: [lists[l][i] for l in range(1, int(levels[i]) + 1)] for i in range(n) if levels[i] >= 1}
    g = H.graph_of(rows, lists[0], upper, entry, keys=keys, m0=p.m0, m=p.m)
    return g, Counters(len(plan), dists[0], requests, prunes)


def recall(found, truth):
    """found, truth: [Q][k] keys"""
    return float(np.mean([len(set(f.tolist()) & set(t.tolist())) / float(len(t)) for f, t in zip(found, truth)]))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def mid_levels(n, sf, seed=3):
    """generated levels with two level-2 nodes and one level-3 node forced into the middle of the sequence"""
    lv = np.minimum(levels_model(n, sf, seed), 1)
    lv[0] = 1
    lv[n // 3] = 2
    lv[n // 2] = 3
    lv[n // 2 + 40] = 2
    return lv


@functools.lru_cache(maxsize=None)
def base_rows(n=600, dim=24, seed=21):
    return H.exact_rows(np.random.default_rng([seed, n, dim]), n, dim)


def base(metric="l2", round_div=16, round_max=64, n=600, dim=24, **kw):
    p = params(m=4, m0=8, ef_construction=16, **kw)
    return Fixture(base_rows(n, dim), p, mid_levels(n, p.scaling_factor), round_div, round_max, metric)


def wide():
    """lists wider than a wave"""
    p = params(m=40, m0=80, ef_construction=100)
    return Fixture(base_rows(300, 24), p, mid_levels(300, 4), 16, 64, "l2")


def all_shortcut():
    """ef_construction < m0 and <= min(prune_cnt, m): every W is taken whole"""
    p = params(m=8, m0=16, ef_construction=6)
    return Fixture(base_rows(600, 24), p, mid_levels(600, 8), 16, 64, "l2")


def duplicates():
    """300 nodes on 40 distinct rows: distance 0 between distinct nodes, the <= of the keep rule decides"""
    rng = np.random.default_rng(31)
    rows = H.exact_rows(rng, 40, 24)[rng.integers(0, 40, 300)]
    p = params(m=4, m0=8, ef_construction=16)
    return Fixture(rows, p, mid_levels(300, 4), 16, 64, "l2")


def line_clusters():
    """three clusters on a line, each node of a round nearest to the same few old nodes: one target receives more requests in a
    round than its list holds"""
    rng = np.random.default_rng(41)
    n = 400
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0] = (np.arange(n) % 3) * 1000 + rng.integers(0, 6, n)
    p = params(m=4, m0=8, ef_construction=16)
    return Fixture(rows, p, mid_levels(n, 4), 1, 64, "l2")


def tiny(n):
    p = params(m=4, m0=8, ef_construction=16)
    return Fixture(base_rows(600, 24)[:n], p, mid_levels(600, 4)[:n], 16, 64, "l2")


SLICED_N, SLICED_ROUND_MAX = 784, 272      # round_div 1: the rounds at 256 and 512 nodes take 256 and 272 nodes


def sliced():
    p = params(m=4, m0=8, ef_construction=16)
    return Fixture(base_rows(SLICED_N, 24), p, np.zeros(SLICED_N, np.uint32), 1, SLICED_ROUND_MAX, "l2")


def slices_of(fx, ws_bytes):
    """the most slices a round's insert phase goes in: a node's share is ceil(s / 32) words of visited bits, and 8 * s bytes of
    candidate region once s > 1024 nodes are in the graph (include/zvec_hip.h)"""
    most = 0
    for s, e, _, _ in rounds_of(fx.levels, fx.round_div, fx.round_max):
        per = 4 * ((s + 31) // 32) + (8 * s if s > H.C_LDS else 0)
        per_slice = max(1, min(e - s, ws_bytes // per))
        most = max(most, -(-(e - s) // per_slice))
    return most


FIXTURES = collections.OrderedDict(
    [("%s-div%d-max%d" % (mt, rd, rm), functools.partial(base, mt, rd, rm)) for mt in ("l2", "ip") for rd in (0, 1, 16) for rm in (7, 64)]
    + [("wide", wide), ("all_shortcut", all_shortcut),
       ("prune_cnt_small", functools.partial(base, prune_cnt=2)), ("prune_cnt_large", functools.partial(base, prune_cnt=12)),
       ("min_neighbors", functools.partial(base, min_neighbors=4)),
       ("dim5", functools.partial(base, dim=5)), ("dim100", functools.partial(base, dim=100)),
       ("duplicates", duplicates), ("line_clusters", line_clusters),
       ("n1", functools.partial(tiny, 1)), ("n2", functools.partial(tiny, 2)), ("n35", functools.partial(tiny, 35)),
       ("sliced", sliced)])
# n35: with round_div 16 a round holds one node until 32 nodes are in the graph; [32, 34) is the first round of two, and node 34
# is alone in the round after it, which the row count cuts short


@functools.lru_cache(maxsize=None)
def model_of(name):
    fx = FIXTURES[name]()
    book = {}
    g, c = build_model(fx.rows, fx.params, fx.levels, fx.round_div, fx.round_max, fx.metric, book=book)
    return fx, g, c, book


# ---- quality on real data ------------------------------------------------------------------------------------------------------
QUALITY_N, QUALITY_DIM, QUALITY_Q, QUALITY_EF, QUALITY_K, QUALITY_SEED = 2000, 16, 100, 32, 10, 77
QUALITY_PARAMS = params(m=8, m0=16, ef_construction=40)
# recall@10 of search_model (ef 32) on the graph the SEQUENTIAL model (one node per round) builds from quality_data(), against
# brute force; recomputed by tests/test_hnsw_build_reference_cpu.py
QUALITY_P = 0.966


@functools.lru_cache(maxsize=None)
def quality_data():
    rng = np.random.default_rng(QUALITY_SEED)
    rows = rng.standard_normal((QUALITY_N, QUALITY_DIM)).astype(np.float32)
    q = rng.standard_normal((QUALITY_Q, QUALITY_DIM)).astype(np.float32)
    levels = levels_model(QUALITY_N, QUALITY_PARAMS.scaling_factor, QUALITY_SEED)
    return rows, q, levels


def quality_truth(rows, q):
    d = ((q.astype(np.float64)[:, None, :] - rows.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, 1, kind="stable")[:, :QUALITY_K].astype(np.uint64)


def quality_floor(p=None):
    """p minus two standard errors of a recall estimated on Q * k pairs"""
    p = QUALITY_P if p is None else p
    return p - 2.0 * (p * (1.0 - p) / (QUALITY_Q * QUALITY_K)) ** 0.5

"""Model, builder and fixtures of the HNSW graph search (zvec_hip_hnsw_*).

search_model is the traversal rule in fp64 numpy: the specification the kernel is compared with, statistic by statistic.
build_graph is a plain HNSW insertion that only has to give valid, well-connected graphs of one to three thousand nodes; nothing
compares it with the reference's builder.  The hand-made graphs are the shapes a builder never gives."""
import bisect
import collections
import functools
import math

import numpy as np

NONE = 0xffffffff
C_LDS = 1024          # candidates the kernel holds in LDS before a query's set moves into the context workspace (zvk_hnsw.hip.h)

Graph = collections.namedtuple("Graph", "rows keys m0 nbr0 cnt0 max_level m n_upper upper_of nbr_up cnt_up entry_point")
Result = collections.namedtuple("Result", "keys scores scanned hops dists evicted on_limit c_peak nodes")


def scores64(rows, q, metric):
    """fp64 scores of one query against rows: squared L2 distance, or minus the dot product"""
    r = np.asarray(rows, np.float64)
    q = np.asarray(q, np.float64)
    if metric == "ip":
        return -(r @ q)
    d = r - q
    return np.einsum("ij,ij->i", d, d)


def graph_of(rows, lists0, upper=None, entry_point=0, keys=None, m0=None, m=None):
    """lists0: the level-0 neighbour list of every node; upper: {node: [list on level 1, list on level 2, ...]}"""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    m0 = m0 or max([len(x) for x in lists0] + [1])
    nbr0 = np.zeros((n, m0), np.uint32)
    cnt0 = np.zeros(n, np.uint32)
    for i, x in enumerate(lists0):
        nbr0[i, :len(x)] = x
        cnt0[i] = len(x)
    upper = upper or {}
    max_level = max([len(v) for v in upper.values()] + [0])
    n_upper = len(upper)
    m = m or max([len(x) for v in upper.values() for x in v] + [1])
    upper_of = np.full(n, NONE, np.uint32)
    nbr_up = np.zeros((max(n_upper, 1), max(max_level, 1), m), np.uint32)
    cnt_up = np.zeros((max(n_upper, 1), max(max_level, 1)), np.uint32)
    for u, node in enumerate(sorted(upper)):
        upper_of[node] = u
        for l, x in enumerate(upper[node]):
            nbr_up[u, l, :len(x)] = x
            cnt_up[u, l] = len(x)
    keys = np.arange(n, dtype=np.uint64) if keys is None else np.ascontiguousarray(keys, np.uint64)
    return Graph(rows, keys, m0, nbr0, cnt0, max_level, m, n_upper, upper_of, nbr_up, cnt_up, int(entry_point))


def check_graph(g):
    """the preconditions zvec_hip_hnsw_load validates"""
    n = g.rows.shape[0]
    assert g.entry_point < n
    assert (g.cnt0 <= g.m0).all()
    for i in range(n):
        assert (g.nbr0[i, :g.cnt0[i]] < n).all()
    if g.max_level >= 1:
        assert g.upper_of[g.entry_point] != NONE
        assert (g.cnt_up <= g.m).all()
        for u in range(g.n_upper):
            for l in range(g.max_level):
                ids = g.nbr_up[u, l, :g.cnt_up[u, l]]
                assert (ids < n).all() and (g.upper_of[ids] != NONE).all()


def search_model(g, q, topk, ef, max_scan=0, threshold=None, exclude=None, metric="l2"):
    """The rule of DESIGN §3c for one query.  exclude: boolean per node or None.  Returns keys, scores (fp32 of the fp64 score),
    distances computed, nodes expanded, the sorted array of every distance computed — and what the fixtures must show: how many
    candidates left a full C, whether the walk ended on the scan limit, the most candidates C ever held, the rows computed."""
    n = g.rows.shape[0]
    if n == 0:
        return Result(np.zeros(0, np.uint64), np.zeros(0, np.float32), 0, 0, np.zeros(0), 0, False, 0, np.zeros(0, np.int64))
    ef = max(int(ef), int(topk))
    max_scan = int(max_scan) or n
    r64 = g.rows.astype(np.float64)
    ex = (lambda i: False) if exclude is None else (lambda i: bool(exclude[i]))
    computed, nodes = [], []

    def dist(ids):
        d = scores64(r64[ids], q, metric) + 0.0
        computed.extend(d.tolist())
        nodes.extend(int(i) for i in ids)
        return d

    ep = g.entry_point
    cur = float(dist([ep])[0])
    scanned = 1
    for level in range(g.max_level, 0, -1):
        while True:
            u = g.upper_of[ep]
            ids = g.nbr_up[u, level - 1, :g.cnt_up[u, level - 1]]
            if ids.size == 0:
                break
            d = dist(ids)
            scanned += ids.size
            moved = False
            for i, di in zip(ids.tolist(), d.tolist()):
                if di < cur:
                    ep, cur, moved = i, di, True
            if not moved:
                break
    visited = np.zeros(n, bool)
    visited[ep] = True
    R = [] if ex(ep) else [(cur, ep)]
    C = [(cur, ep)]
    hops = evicted = 0
    c_peak = 1
    while C and scanned < max_scan:
        dc, c = C[0]
        if len(R) == ef and dc > R[-1][0]:
            break
        C.pop(0)
        hops += 1
        coll = []
        for v in g.nbr0[c, :g.cnt0[c]].tolist():
            if not visited[v]:
                visited[v] = True
                coll.append(v)
        if not coll:
            continue
        d = dist(coll)
        scanned += len(coll)
        for v, dv in zip(coll, d.tolist()):
            if len(R) < ef or dv < R[-1][0]:
                bisect.insort(C, (dv, v))
                if len(C) > max_scan:
                    C.pop()
                    evicted += 1
                c_peak = max(c_peak, len(C))
                if not ex(v):
                    bisect.insort(R, (dv, v))
                    if len(R) > ef:
                        R.pop()
    on_limit = bool(C) and scanned >= max_scan
    out = [(d, v) for d, v in R[:topk] if threshold is None or np.float32(d) <= np.float32(threshold)]
    keys = np.array([g.keys[v] for _, v in out], np.uint64)
    scores = np.array([d for d, _ in out], np.float32)
    return Result(keys, scores, scanned, hops, np.sort(np.array(computed)), evicted, on_limit, c_peak, np.array(nodes, np.int64))


def brute_force(g, q, topk, metric="l2", exclude=None):
    d = scores64(g.rows, q, metric) + 0.0
    order = sorted((float(d[i]), i) for i in range(len(d)) if exclude is None or not exclude[i])[:topk]
    return np.array([g.keys[i] for _, i in order], np.uint64), np.array([s for s, _ in order], np.float32)


def reachable(g):
    """nodes a level-0 walk from the entry point's component can see (the entry point of level 0 is in that component)"""
    seen = {g.entry_point}
    todo = [g.entry_point]
    while todo:
        c = todo.pop()
        for v in g.nbr0[c, :g.cnt0[c]].tolist():
            if v not in seen:
                seen.add(v)
                todo.append(v)
    return seen


# ---- builder ---------------------------------------------------------------------------------------------------------------
def _prune(cands, D, cap):
    """the HNSW selection heuristic: walk the candidates nearest first and keep one unless a kept node is at least as near to it
    as the base is"""
    kept = []
    for d, v in cands:
        if all(D[v, s] > d for s in kept):
            kept.append(v)
            if len(kept) >= cap:
                break
    return kept


def _search_layer(D, lists, q, ep, ef):
    """search_neighbors on one level of the graph under construction: the ef nearest of q's row found from ep, sorted"""
    visited = {ep}
    R = [(D[q, ep], ep)]
    C = [(D[q, ep], ep)]
    while C:
        dc, c = C.pop(0)
        if len(R) == ef and dc > R[-1][0]:
            break
        for v in lists[c]:
            if v in visited:
                continue
            visited.add(v)
            dv = D[q, v]
            if len(R) < ef or dv < R[-1][0]:
                bisect.insort(C, (dv, v))
                bisect.insort(R, (dv, v))
                if len(R) > ef:
                    R.pop()
    return R


def build_graph(rows, m, efc, seed, metric="l2"):
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    r64 = rows.astype(np.float64)
    if metric == "ip":
        D = -(r64 @ r64.T)
    else:
        sq = np.einsum("ij,ij->i", r64, r64)
        D = sq[:, None] + sq[None, :] - 2.0 * (r64 @ r64.T)
    rng = np.random.default_rng(seed)
    levels = np.minimum((-np.log(1.0 - rng.random(n)) / math.log(m)).astype(np.int64), 4)
    m0 = 2 * m
    lists = [[[] for _ in range(n)] for _ in range(int(levels.max()) + 1)]
    entry, top = 0, int(levels[0])
    for i in range(1, n):
        li = int(levels[i])
        ep = entry
        for level in range(top, li, -1):
            moved = True
            while moved:
                moved = False
                for v in lists[level][ep]:
                    if D[i, v] < D[i, ep]:
                        ep, moved = v, True
        for level in range(min(li, top), -1, -1):
            cap = m0 if level == 0 else m
            W = _search_layer(D, lists[level], i, ep, efc)
            sel = _prune(W, D, cap)
            lists[level][i] = list(sel)
            for s in sel:
                back = lists[level][s]
                back.append(i)
                if len(back) > cap:
                    lists[level][s] = _prune(sorted((D[s, v], v) for v in back), D, cap)
            ep = W[0][1]
        if li > top:
            entry, top = i, li
    # pruning a back-link may leave a node that nobody names: give each such node to the nearest reachable node with room
    while True:
        seen = {entry}
        todo = [entry]
        while todo:
            for v in lists[0][todo.pop()]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        lost = [i for i in range(n) if i not in seen]
        if not lost:
            break
        u = lost[0]
        room = [v for v in seen if len(lists[0][v]) < m0]
        lists[0][min(room, key=lambda v: (D[u, v], v))].append(u)
    upper = {i: [lists[l][i] for l in range(1, int(levels[i]) + 1)] for i in range(n) if levels[i] >= 1}
    g = graph_of(rows, lists[0], upper, entry, m0=m0, m=m)
    return g._replace(keys=(np.arange(n, dtype=np.uint64) * 7 + 3))


# ---- data ------------------------------------------------------------------------------------------------------------------
def exact_rows(rng, n, dim):
    """integer values in [-8, 8]: every distance is an exact fp32 integer in any summation order (dim <= 128), ties are plentiful"""
    assert dim <= 128
    return rng.integers(-8, 9, (n, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_graph(n, dim, m, seed=5):
    rng = np.random.default_rng([seed, n, dim, m])
    rows = exact_rows(rng, n, dim)
    return build_graph(rows, m, 24, seed)


def exact_queries(g, rng, count):
    """random queries; a few are rows of the graph"""
    q = exact_rows(rng, count, g.rows.shape[1])
    if count >= 3:
        q[1] = g.rows[rng.integers(0, g.rows.shape[0])]
    return q


# seeds of the committed real-data fixtures: the model alone shows that at least 3/4 of each one's queries are decisive
# (31 and 26 of 32).  A walk that computes N distances has N^2 / 2 pairs of them to keep 2 * band apart, so the walks are short: m = 4
# and ef = 4 compute about 65 distances a query.
REAL = {32: 11, 96: 12}
REAL_N, REAL_Q, REAL_M, REAL_EF, REAL_TOPK = 2000, 32, 4, 4, 4


@functools.lru_cache(maxsize=None)
def real_graph(dim):
    rng = np.random.default_rng(REAL[dim])
    rows = rng.standard_normal((REAL_N, dim)).astype(np.float32)
    q = rng.standard_normal((REAL_Q, dim)).astype(np.float32)
    return build_graph(rows, REAL_M, 24, REAL[dim]), q


def band(g, q, ids):
    """accumulation slack of an fp32 score of q: (dim + 8) * 2^-23 * max over the computed rows `ids` of (|q|^2 + |b|^2)"""
    r = g.rows[ids].astype(np.float64)
    q = np.asarray(q, np.float64)
    return (g.rows.shape[1] + 8) * 2.0 ** -23 * float((q @ q + np.einsum("ij,ij->i", r, r)).max())


def decisive(res, b, threshold=None):
    """no two distinct distances the model computed, and no distance and the threshold, are within 2 * band"""
    d = np.unique(res.dists)
    if d.size > 1 and np.diff(d).min() <= 2 * b:
        return False
    return threshold is None or np.abs(d - threshold).min() > 2 * b


# ---- hand-made graphs --------------------------------------------------------------------------------------------------------
def _line_rows(n, dim=4):
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = np.arange(n)
    return rows


def chain(n=40):
    """0 - 1 - ... - n-1 along a line; entry point 0"""
    return graph_of(_line_rows(n), [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)])


def star(n=70):
    """node 0 at the origin sees everybody (more neighbours than lanes), everybody sees node 0 only; rows on a line"""
    return graph_of(_line_rows(n), [list(range(1, n))] + [[0]] * (n - 1))


def two_components():
    """nodes 0..4 (entry point 2) and 5..19 are not connected; the query sits in the larger component"""
    rows = _line_rows(20)
    lists = [[j for j in (i - 1, i + 1) if 0 <= j < 5] for i in range(5)] + [[j for j in (i - 1, i + 1) if 5 <= j < 20] for i in range(5, 20)]
    return graph_of(rows, lists, entry_point=2)


def with_empty_lists():
    """a chain whose nodes 3 and 6 have no neighbours (dead ends that are still reached)"""
    n = 10
    lists = [[j for j in (i - 1, i + 1, i + 2) if 0 <= j < n] for i in range(n)]
    lists[3] = []
    lists[6] = []
    return graph_of(_line_rows(n), lists)


def bare_upper():
    """two upper levels; node 9 is on level 2 with no upper neighbours at all, node 4 on level 1 with none on level 1"""
    n = 12
    lists = [[j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)]
    upper = {0: [[4, 7], [9]], 9: [[], []], 4: [[]], 7: [[0, 4]]}
    return graph_of(_line_rows(n), lists, upper, entry_point=0)


def single():
    return graph_of(_line_rows(1), [[]])


def duplicate_ids():
    """every list names a neighbour twice, once with another node in between"""
    n = 8
    lists = [[(i + 1) % n, (i + 3) % n, (i + 1) % n, (i + 3) % n, (i + 5) % n] for i in range(n)]
    rows = _line_rows(n)
    rows[:, 1] = [0, 2, 0, 2, 0, 2, 0, 2]
    return graph_of(rows, lists)


def tie_ring(n=64):
    """a ring with chords whose rows repeat four times over: every distance ties four ways"""
    rows = np.zeros((n, 4), np.float32)
    rows[:, 0] = np.arange(n) % 16
    rows[:, 1] = (np.arange(n) % 16) // 4
    lists = [[(i + 1) % n, (i - 1) % n, (i + 7) % n, (i + 16) % n] for i in range(n)]
    return graph_of(rows, lists, upper={0: [[32]], 32: [[0]]}, entry_point=0)


HAND_MADE = collections.OrderedDict([("chain", chain), ("star", star), ("two_components", two_components),
                                     ("with_empty_lists", with_empty_lists), ("bare_upper", bare_upper), ("single", single),
                                     ("duplicate_ids", duplicate_ids), ("tie_ring", tie_ring)])


def words_of(mask):
    """a boolean per node -> the uint64 words of an exclude bitset"""
    mask = np.asarray(mask, bool)
    out = np.zeros((mask.size + 63) // 64, np.uint64)
    for i in np.nonzero(mask)[0].tolist():
        out[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return out

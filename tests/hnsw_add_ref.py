"""Model and fixtures of appending to an HNSW graph (zvec_hip_hnsw_add, DESIGN §3c "Appending").

add_model is the loop of hnsw_build_ref.build_model over a plan that is restarted at every call boundary: the first call is the build
(node 0 is the seed), every later call inserts its rows by rounds that start at s = the nodes already there.  It returns the graph and
the counters after every call.  The fixtures are the shapes at which an append takes each of its paths;
tests/test_hnsw_add_reference_cpu.py asserts from the model's own bookkeeping that they do."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402
from hnsw_build_ref import distance_matrix, keep_rule, search_level  # noqa: E402
from hnsw_ref import graph_of  # noqa: E402

Call = collections.namedtuple("Call", "first count graph counters restrided book")
Fixture = collections.namedtuple("Fixture", "rows params levels calls round_div round_max metric")


def rounds_from(levels, base, end, entry, top, round_div, round_max):
    """[(first, end, entry point, top level)] of the rounds that insert the nodes base .. end - 1 into a graph of base nodes with the
    given entry point and top level, and (entry, top) after them; base == 0: node 0 is the seed"""
    out = []
    s = base
    if base == 0:
        entry, top, s = 0, int(levels[0]) if end else 0, 1
    while s < end:
        if levels[s] > top:
            out.append((s, s + 1, entry, top))
            entry, top = s, int(levels[s])
            s += 1
            continue
        size = 1 if round_div == 0 else min(max(s // round_div, 1), round_max)
        e = min(s + size, end)
        for j in range(s + 1, e):
            if levels[j] > top:
                e = j
                break
        out.append((s, e, entry, top))
        s = e
    return out, entry, top


def add_model(rows, p, levels, calls, round_div=16, round_max=4096, metric="l2", keys=None):
    """calls: the rows of every call in order, the first on an empty handle.  Returns [Call]: the graph (hnsw_ref.Graph) after the
    call, the Counters of the call alone, whether the call raised the largest level (the upper table is re-strided or made), and a
    book: round sizes, rounds of one node, own rounds with their place in the call, prunes that dropped a link the target had before
    the CALL, the most nodes in the graph when a round began, prunes run and lists of 64 or more
    ids met by rounds of one node."""
    rows = np.ascontiguousarray(rows, np.float32)
    levels = np.asarray(levels, np.uint32)
    n = rows.shape[0]
    assert sum(calls) == n and all(c > 0 for c in calls)
    D = distance_matrix(rows, metric)
    nlev = int(levels.max()) + 1
    lists = [[[] for _ in range(n)] for _ in range(nlev)]
    out = []
    base, entry, top, stride = 0, 0, 0, 0
    for count in calls:
        end = base + count
        plan, new_entry, new_top = rounds_from(levels, base, end, entry, top, round_div, round_max)
        before = [[set(x) for x in lv[:base]] for lv in lists]
        bk = dict(round_sizes=[], one_rounds=0, own_rounds=[], dropped_old_links=0, max_s=0, prunes_one=0, long_one=0)
        dists = [0]
        requests = prunes = 0
        for s, e, entry, top in plan:
            bk["round_sizes"].append(e - s)
            bk["one_rounds"] += e - s == 1
            bk["max_s"] = max(bk["max_s"], s)
            if levels[s] > top:
                bk["own_rounds"].append(s - base)
            reqs, own = [], []
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
                    if len(W) <= min(p.prune_cnt, cap):
                        sel = [v for _, v in W]
                    else:
                        sel = keep_rule(W, D, cap, dists)
                        for _, v in W:
                            if len(sel) >= p.min_neighbors:
                                break
                            if v not in sel:
                                sel.append(v)
                    own.append((level, i, sel))
                    reqs.extend((level, t, i) for t in sel)
            for level, i, sel in own:
                lists[level][i] = list(sel)
            requests += len(reqs)
            for level, t, i in sorted(reqs):
                cap = p.m0 if level == 0 else p.m
                lst = lists[level][t]
                bk["long_one"] += e - s == 1 and len(lst) >= 64
                if len(lst) < cap:
                    lst.append(i)
                    continue
                prunes += 1
                bk["prunes_one"] += e - s == 1
                kept = keep_rule(sorted((D[t, x], x) for x in lst + [i]), D, cap)
                if t < base and any(x in before[level][t] and x not in kept for x in lst):
                    bk["dropped_old_links"] += 1
                lists[level][t] = kept
        entry, top = new_entry, new_top
        new_stride = int(levels[:end].max())
        upper = {i: [list(lists[l][i]) for l in range(1, int(levels[i]) + 1)] for i in range(end) if levels[i] >= 1}
        g = graph_of(rows[:end], [list(x) for x in lists[0][:end]], upper, entry, keys=None if keys is None else keys[:end], m0=p.m0, m=p.m)
        out.append(Call(base, count, g, B.Counters(len(plan), dists[0], requests, prunes), new_stride > stride, bk))
        base, stride = end, new_stride
    return out


def slices_of(fx, call, ws_bytes):
    """the most slices the insert phase of a round of call number `call` goes in (hnsw_build_ref.slices_of, from a base)"""
    base = sum(fx.calls[:call])
    entry, top = 0, 0
    if base:
        _, entry, top = rounds_from(fx.levels, 0, base, 0, 0, fx.round_div, fx.round_max)
        # (the rounds of the calls before: only the entry point and the top level they leave matter, and those do not depend on the cuts)
    plan, _, _ = rounds_from(fx.levels, base, base + fx.calls[call], entry, top, fx.round_div, fx.round_max)
    most = 0
    for s, e, _, _ in plan:
        per = 4 * ((s + 31) // 32) + (8 * s if s > H.C_LDS else 0)
        per_slice = max(1, min(e - s, ws_bytes // per))
        most = max(most, -(-(e - s) // per_slice))
    return most


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def cut(metric="l2"):
    """cuts inside what one build would make one round"""
    fx = B.base(metric, 16, 64)
    return Fixture(fx.rows, fx.params, fx.levels, (200, 37, 1, 150, 212), 16, 64, metric)


def top_raised():
    """largest level 1 after the build; a level-3 node in the middle of the second call (stride 1 -> 3, an own round inside a call),
    a level-2 node first in the third"""
    p = B.params(m=4, m0=8, ef_construction=16)
    lv = np.minimum(B.levels_model(350, 4, 3), 1)
    lv[0] = 1
    lv[200] = 3
    lv[250] = 2
    return Fixture(B.base_rows(600, 24)[:350], p, lv, (150, 100, 100), 16, 64, "l2")


def first_upper():
    """100 rows at level 0 built; the add makes the upper arrays (a level-1 node, then a level-2 node), a later call adds to them"""
    p = B.params(m=4, m0=8, ef_construction=16)
    lv = np.zeros(200, np.uint32)
    lv[[120, 130, 170]] = 1
    lv[140] = 2
    return Fixture(B.base_rows(600, 24)[:200], p, lv, (100, 60, 40), 16, 64, "l2")


def prune_old():
    """the line_clusters rows: appended nodes push links out of lists that were full before the call"""
    fx = B.line_clusters()
    return Fixture(fx.rows, fx.params, fx.levels, (250, 150), fx.round_div, fx.round_max, fx.metric)


def wide():
    """lists wider than a wave (80 and 40 places; a node has 80 request slots and more), through a call of 90 rows and ten calls of
    one row (the one-node path), which meet lists of 64 ids and more.  300 rows fill no list of 80, so no prune runs at that width"""
    fx = B.wide()
    return Fixture(fx.rows, fx.params, fx.levels, (200, 90) + (1,) * 10, fx.round_div, fx.round_max, fx.metric)


SPILL_N, SPILL_BUILT, SPILL_ROUND_MAX = 1100, 1030, 34       # the add's rounds take 34, 34 and 2 nodes at s = 1030, 1064, 1098


def spill():
    """more than 1024 nodes in the graph when the add begins: the candidate regions are in workspace"""
    p = B.params(m=4, m0=8, ef_construction=16)
    return Fixture(B.base_rows(SPILL_N, 24), p, np.zeros(SPILL_N, np.uint32), (SPILL_BUILT, SPILL_N - SPILL_BUILT), 16, SPILL_ROUND_MAX, "l2")


FIXTURES = collections.OrderedDict([("cut", cut), ("top_raised", top_raised), ("first_upper", first_upper), ("prune_old", prune_old),
                                    ("wide", wide), ("spill", spill), ("ip", functools.partial(cut, "ip"))])


def _keys(n):
    return np.arange(n, dtype=np.uint64) * 7 + 3


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(fixture, [Call]) with the keys the GPU tests give their rows"""
    fx = FIXTURES[name]()
    return fx, add_model(fx.rows, fx.params, fx.levels, fx.calls, fx.round_div, fx.round_max, fx.metric, keys=_keys(fx.rows.shape[0]))

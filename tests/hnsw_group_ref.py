"""Model of the group-by search on an HNSW graph (zvec_hip_hnsw_search_grouped, DESIGN §3c "Group-by") in fp64, the brute force it
must equal on a connected graph walked whole, and the fixtures of its tests with the fact each exists for."""
import bisect
import collections

import numpy as np

import hnsw_ref as H

NONE = 0xffffffff
GroupResult = collections.namedtuple("GroupResult", "groups keys scores counts scanned hops expanded ended inserted_before")
Case = collections.namedtuple("Case", "g q group_of ngroups group_num group_topk ef max_scan threshold exclude metric fact")


def _finish(g, slots, group_num, threshold, scanned=0, hops=0, expanded=False, ended=None, before=0):
    """G4: slots {group: ascending [(d, node)]} -> the first group_num groups by best document"""
    top = sorted(slots.items(), key=lambda kv: kv[1][0])[:group_num]
    within = lambda d: threshold is None or np.float32(d) <= np.float32(threshold)
    return GroupResult([k for k, _ in top], [np.array([g.keys[v] for _, v in docs], np.uint64) for _, docs in top],
                       [np.array([d for d, _ in docs], np.float32) for _, docs in top],
                       [sum(within(d) for d, _ in docs) for _, docs in top], scanned, hops, expanded, ended, before)


def group_search_model(g, q, group_of, ngroups, group_num, group_topk, ef, max_scan=0, threshold=None, exclude=None, metric="l2"):
    n = g.rows.shape[0]
    if n == 0:
        return _finish(g, {}, group_num, threshold)
    ef_eff = max(int(ef), group_num * group_topk)
    max_scan = int(max_scan) or n
    d_all = H.scores64(g.rows, q, metric) + 0.0
    # G1: steps 1-3 of the plain rule; with positions as keys the result list is R itself
    res = H.search_model(g._replace(keys=np.arange(n, dtype=np.uint64)), q, ef_eff, ef_eff, max_scan, None, exclude, metric)
    R = [(float(d_all[int(v)]), int(v)) for v in res.keys]
    scanned, hops, slots, before = res.scanned, res.hops, {}, 0

    def offer(d, v):                                 # True when the document went in front of an earlier one of its slot
        if int(group_of[v]) not in slots and len(slots) == group_num:
            return False
        docs = slots.setdefault(int(group_of[v]), [])
        at = bisect.bisect(docs, (d, v))
        front = at < min(len(docs), group_topk)
        docs.insert(at, (d, v))
        del docs[group_topk:]
        return front

    for d, v in R:                                   # G2
        if group_of[v] < ngroups:
            offer(d, v)
    if len(slots) >= group_num:
        return _finish(g, slots, group_num, threshold, scanned, hops)
    visited = np.zeros(n, bool)                      # G3
    visited[[v for _, v in R]] = True
    C, ended = list(R), None
    while ended is None and C and scanned < max_scan:
        _, c = C.pop(0)
        hops += 1
        coll = [v for v in dict.fromkeys(g.nbr0[c, :g.cnt0[c]].tolist()) if not visited[v]]
        visited[coll] = True
        for v in coll:
            scanned += 1
            d = float(d_all[v])
            if (exclude is None or not exclude[v]) and group_of[v] < ngroups:
                before += offer(d, v)
                if len(slots) == group_num:
                    ended = "groups"
                    break
            bisect.insort(C, (d, v))
            del C[max_scan:]
    return _finish(g, slots, group_num, threshold, scanned, hops, True, ended or ("limit" if C else "empty"), before)


def brute_force_grouped(g, q, group_of, ngroups, group_num, group_topk, exclude=None, metric="l2"):
    d = H.scores64(g.rows, q, metric) + 0.0
    ok = np.ones(len(d), bool) if exclude is None else ~np.asarray(exclude, bool)
    slots = {k: sorted((float(d[v]), int(v)) for v in np.nonzero(ok & (group_of == k))[0])[:group_topk] for k in range(ngroups)}
    return _finish(g, {k: docs for k, docs in slots.items() if docs}, group_num, None)


def model_of(c):
    return [group_search_model(c.g, q, c.group_of, c.ngroups, c.group_num, c.group_topk, c.ef, c.max_scan, c.threshold, c.exclude, c.metric)
            for q in c.q]


def _case(g, q, group_of, group_num, group_topk, ef, fact, ngroups=None, max_scan=0, threshold=None, exclude=None, metric="l2"):
    group_of = np.asarray(group_of, np.uint32)
    return Case(g, np.atleast_2d(np.asarray(q, np.float32)), group_of, ngroups or int(group_of[group_of != NONE].max()) + 1, group_num,
                group_topk, ef, max_scan, threshold, exclude, metric, fact)


def cases():
    """name -> Case; fact: a predicate on the model's results of the case's queries"""
    out = collections.OrderedDict()
    big = H.exact_graph(600, 16, 8)
    qs = H.exact_queries(big, np.random.default_rng(3), 40)
    mod7 = np.arange(600) % 7
    plain = lambda ms: sum(not m.expanded for m in ms) >= len(ms) // 2
    ends = lambda why: lambda ms: all(m.expanded and m.ended == why for m in ms)
    for name, gnum, gk, ef in (("3x2_ef4", 3, 2, 4), ("3x2_ef40", 3, 2, 40), ("7x4_ef9", 7, 4, 9), ("7x4_ef60", 7, 4, 60)):
        out[name] = _case(big, qs, mod7, gnum, gk, ef, plain)
    # (with ef 40, R holds more groups than the three asked for: asked for all seven, it has them without expansion)
    wide = lambda ms: plain(ms) and all(len(m.groups) == 7 and not m.expanded for m in model_of(out["3x2_ef40"]._replace(group_num=7, group_topk=1)))
    out["3x2_ef40"] = out["3x2_ef40"]._replace(fact=wide)
    out["ip"] = _case(big, qs[:8], mod7, 3, 2, 12, plain, metric="ip")
    out["excluded_nogroup"] = _case(big, qs[:8], np.where(np.arange(600) % 5 == 0, NONE, mod7), 7, 4, 40, plain, ngroups=7,
                                    exclude=np.arange(600) % 3 == 1)
    # a chain walked from node 0 towards the only node of the last group, at its far end (G3 scores again what G1 scored beyond R:
    # the scan limit is set above the node count); the threshold lies between the two groups
    n, q0 = 40, np.zeros(4)
    far = np.where(np.arange(n) == n - 1, 1, 0)
    out["chain_groups"] = _case(H.chain(n), q0, far, 2, 2, 2, lambda ms: ends("groups")(ms) and ms[0].counts == [2, 0], max_scan=100, threshold=100.0)
    out["chain_limit"] = _case(H.chain(n), q0, far, 2, 2, 2, ends("limit"), max_scan=20)
    walked = far.copy()
    walked[[20, 36, 30, 38]] = (NONE, 5, 1, 1)       # 20, 36: no group; 30, 38: excluded below; all walked through, none ends the stage
    out["chain_walked_through"] = _case(H.chain(n), q0, walked, 2, 2, 2, lambda ms: ends("groups")(ms) and ms[0].keys[1].tolist() == [n - 1],
                                        ngroups=2, max_scan=100, exclude=np.isin(np.arange(n), (10, 30, 38)))
    # even nodes also see two ahead, and name the farther neighbour first: node 6 finds 8 and then 7 for the middle group
    jump = H.graph_of(H._line_rows(n), [[j for j in ((i + 2,) if i % 2 == 0 else ()) + (i + 1, i - 1) if 0 <= j < n] for i in range(n)])
    mid = np.where(np.arange(n) > 6, 1, 0) + (np.arange(n) == n - 1)
    out["chain_insert_in_front"] = _case(jump, q0, mid, 3, 2, 7, lambda ms: ends("groups")(ms) and ms[0].inserted_before > 0, max_scan=100)
    out["two_components_empty"] = _case(H.two_components(), [12, 0, 0, 0], np.arange(20) // 5, 2, 2, 2,
                                        lambda ms: ends("empty")(ms) and len(ms[0].groups) == 1)
    return out

"""fp64 reference and the two checkers of group-by search over sparse rows (numpy only), on top of tests/sparse_ref.py.

The rules (include/zvec_hip.h, "Group-by" of the sparse section; FlatSparseEntity::search_group / search_group_p_keys and
ConvertGroupMapToResult in the reference):
  - the score of (query, row) is MINUS the inner product over shared indices; no shared index: exactly +0, an ordinary candidate
  - a position competes iff it is < n, not excluded and has group_of[pos] < ngroups; `candidates` (listed rows): per query the
    positions in list order, a position named twice competes twice, each time with its own ordinal
  - a group keeps its gk best candidates under (score, scan ordinal); ordinal = storage position (full scan) or place in the list
  - groups are ranked by (best score, group number) and the first gnum are kept
  - documents with score > threshold are cut AFTER that ranking: a group may be listed with no document

select() works on any [nq][n] score matrix, so the same code ranks the fp64 reference, an integer matrix, or a deliberately wrong
one (half-accumulated scores).  group_reference() has the dict shape of tests/util.py group_reference, with the sparse band B =
(m + 1) * 2^-23 * A of sparse_ref in place of the dense E.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_ref as R  # noqa: E402

IDX_NONE = 0xffffffff
NO_KEY = 0xffffffffffffffff


def select(scores, group_of, ngroups, gnum, gk, threshold=None, exclude=None, candidates=None):
    """per query a dict
         groups  [(g, positions, scores)]: the listed groups in order, documents after the radius cut
         order   {g: (scores, positions)} of EVERY admissible group: its full ascending (score, ordinal) order
         bests   (scores, group numbers) of every admissible group, ascending (best score, group number)"""
    scores = np.asarray(scores)
    nq, n = scores.shape
    gof = np.asarray(group_of).astype(np.int64)
    live = gof < ngroups
    if exclude is not None:
        live = live & ~np.asarray(exclude, bool)
    out = []
    for qi in range(nq):
        if candidates is None:
            pos = np.nonzero(live)[0]
        else:
            pos = np.asarray(candidates[qi], np.int64).reshape(-1)
            pos = pos[pos < n]
            pos = pos[live[pos]]
        # pos is in scan order: two stable sorts give (group, score, ordinal)
        o1 = np.argsort(scores[qi, pos], kind="stable")
        o2 = np.argsort(gof[pos[o1]], kind="stable")
        pos = pos[o1][o2]
        sc, gg = scores[qi, pos], gof[pos]
        starts = np.nonzero(np.r_[True, gg[1:] != gg[:-1]])[0] if pos.size else np.zeros(0, np.int64)
        ends = np.r_[starts[1:], pos.size]
        order = {int(gg[a]): (sc[a:b], pos[a:b]) for a, b in zip(starts, ends)}
        bg = gg[starts] if pos.size else np.zeros(0, np.int64)
        bs = sc[starts] if pos.size else np.zeros(0)
        rank = np.lexsort((bg, bs))
        groups = []
        for g in bg[rank][:gnum]:
            s, p = order[int(g)]
            s, p = s[:gk], p[:gk]
            if threshold is not None:
                keep = ~(s.astype(np.float32) > np.float32(threshold))
                s, p = s[keep], p[keep]
            groups.append((int(g), p, s))
        out.append({"groups": groups, "order": order, "bests": (bs[rank], bg[rank])})
    return out


def group_reference(case, group_of, ngroups, gnum, gk, threshold=None, exclude=None, candidates=None, queries=None):
    """case: (rows, queries, ref, A, m) as sparse_ref.make_case gives it; `queries`: the query numbers to take (default all).
    Returns {"s64", "B", "m": [nq][n], "queries": select(...)}"""
    ref, A, m = case[2], case[3], case[4]
    if queries is not None:
        ref, A, m = ref[queries], A[queries], m[queries]
    B = (m + 1) * 2.0 ** -23 * A
    return {"s64": ref, "B": B, "m": m,
            "queries": select(ref, group_of, ngroups, gnum, gk, threshold, exclude, candidates)}


def render(selected, gnum, gk, key_of):
    """select()'s answer in the layout of the C ABI: (groups [nq][gnum], ngroups [nq], keys [nq][gnum][gk], scores, counts
    [nq][gnum]); unused slots hold IDX_NONE / the all-ones key / +inf / 0"""
    nq = len(selected)
    key_of = np.asarray(key_of, np.uint64)
    groups = np.full((nq, gnum), IDX_NONE, np.uint32)
    ngroups = np.zeros(nq, np.uint32)
    keys = np.full((nq, gnum, gk), NO_KEY, np.uint64)
    scores = np.full((nq, gnum, gk), np.inf, np.float32)
    counts = np.zeros((nq, gnum), np.uint32)
    for q, rq in enumerate(selected):
        ngroups[q] = len(rq["groups"])
        for i, (g, p, s) in enumerate(rq["groups"]):
            groups[q, i] = g
            counts[q, i] = len(p)
            keys[q, i, :len(p)] = key_of[p]
            scores[q, i, :len(p)] = s
    return groups, ngroups, keys, scores, counts


def check_exact(want, got, what=""):
    """bit for bit: the number of groups, the groups in order, the count of every listed group, its keys in order and the bits
    of its scores.  want, got: (groups, ngroups, keys, scores, counts) as render() lays them out; slots beyond what is listed
    are not compared."""
    wg, wn, wk, ws, wc = want
    gg, gn, gkeys, gs, gc = [np.asarray(a) for a in got]
    assert np.array_equal(gn.astype(np.int64), wn.astype(np.int64)), "%s: groups listed\n got %r\nwant %r" % (what, gn, wn)
    for q in range(len(wn)):
        ng = int(wn[q])
        assert np.array_equal(gg[q, :ng], wg[q, :ng]), "%s query %d: groups\n got %r\nwant %r" % (what, q, gg[q, :ng], wg[q, :ng])
        assert np.array_equal(gc[q, :ng], wc[q, :ng]), "%s query %d: counts\n got %r\nwant %r" % (what, q, gc[q, :ng], wc[q, :ng])
        listed = np.arange(wk.shape[2])[None, :] < wc[q, :ng, None]
        a, b = gkeys[q, :ng][listed], wk[q, :ng][listed]
        assert np.array_equal(a, b), "%s query %d: documents differ at %r" % (what, q, np.nonzero(a != b)[0][:5])
        a = np.ascontiguousarray(gs[q, :ng], np.float32).view(np.uint32)[listed]
        b = np.ascontiguousarray(ws[q, :ng], np.float32).view(np.uint32)[listed]
        assert np.array_equal(a, b), "%s query %d: score bits differ at %r" % (what, q, np.nonzero(a != b)[0][:5])


def check_band(ref, qi, groups, ngroups_out, keys, scores, counts, gnum, gk, pos_of_key, what=""):
    """one query of a full-scan group-by answer on REAL-VALUED data (no radius), accepted as tests/util.py check_groups_band
    accepts a dense one, with s64 / B / m of group_reference:
      documents  a returned document x of group g is accepted iff s64(x) - s64(gk-th of g) <= B(x) + B(gk-th); the list holds
                 min(gk, size of g) distinct admissible members of g, in ascending order of the returned score
      groups     a listed group g is accepted iff best(g) - best(gnum-th group) <= B(best doc of g) + B(best doc of the gnum-th)
      scores     within B of s64 (the scores are final: nothing is re-scored), and exactly 0 where m == 0
    Returns (lists that differ from the fp64 set, ambiguous lists, cut lists, group list differs, group cut ambiguous)."""
    rq, s64, B, m = ref["queries"][qi], ref["s64"][qi], ref["B"][qi], ref["m"][qi]
    bs, bg = rq["bests"]
    nlist = min(gnum, len(bg))
    assert int(ngroups_out) == nlist, "%s: %d groups listed, reference %d" % (what, ngroups_out, nlist)
    got = [int(g) for g in groups[:nlist]]
    assert len(set(got)) == len(got), "%s: a group is listed twice" % what
    bbest = lambda g: B[rq["order"][g][1][0]]
    gamb = False
    if len(bg) > gnum:
        last, nxt = int(bg[gnum - 1]), int(bg[gnum])
        gamb = bs[gnum] - bs[gnum - 1] <= bbest(last) + bbest(nxt)
    ndiff = namb = ncut = 0
    for i, g in enumerate(got):
        assert g in rq["order"], "%s place %d: group %d has no admissible member" % (what, i, g)
        s, p = rq["order"][g]
        last = int(bg[nlist - 1])
        assert s[0] - bs[nlist - 1] <= bbest(g) + bbest(last), "%s: group %d (best %r) listed, rank-gnum best %r, bounds %r %r" % (
            what, g, s[0], bs[nlist - 1], bbest(g), bbest(last))
        c = int(counts[i])
        assert c == min(gk, len(p)), "%s group %d: %d documents of %d members" % (what, g, c, len(p))
        x = np.array([pos_of_key[int(k)] for k in keys[i][:c]], np.int64)
        assert len(set(x.tolist())) == c, "%s group %d: a document twice" % (what, g)
        member = set(p.tolist())
        assert all(int(v) in member for v in x), "%s group %d: a document of another group or an excluded one" % (what, g)
        kth = p[c - 1]
        exc = s64[x] - s64[kth] - B[x] - B[kth]
        assert np.all(exc <= 0), "%s group %d: document %d outside the band by %r" % (what, g, x[np.argmax(exc)], exc.max())
        gs = np.asarray(scores[i][:c], np.float64)
        assert np.all(np.diff(gs) >= 0), "%s group %d: scores not ascending" % (what, g)
        err = np.abs(gs - s64[x])
        assert np.all(err <= B[x]), "%s group %d: score off by %r, bound %r" % (what, g, err.max(), B[x][np.argmax(err - B[x])])
        assert np.all(gs[m[x] == 0] == 0.0), "%s group %d: a pair without a shared index does not score 0" % (what, g)
        if len(p) > gk:
            ncut += 1
            namb += bool(s[gk] - s[gk - 1] <= B[p[gk]] + B[p[gk - 1]])
            ndiff += set(x.tolist()) != set(p[:gk].tolist())
    return ndiff, namb, ncut, set(got) != set(int(g) for g in bg[:nlist]), bool(gamb)


def ambiguity(ref, gnum, gk):
    """(ambiguous, decided) under the reference alone: lists whose gap between ranks gk and gk + 1 is within the two bounds plus
    group cuts whose gap between the best scores at ranks gnum and gnum + 1 is, over all cut lists of listed groups plus all group
    cuts"""
    amb = tot = 0
    for qi, rq in enumerate(ref["queries"]):
        B = ref["B"][qi]
        bs, bg = rq["bests"]
        if len(bg) > gnum:
            tot += 1
            a, b = rq["order"][int(bg[gnum - 1])][1][0], rq["order"][int(bg[gnum])][1][0]
            amb += bool(bs[gnum] - bs[gnum - 1] <= B[a] + B[b])
        for g in bg[:gnum]:
            s, p = rq["order"][int(g)]
            if len(p) > gk:
                tot += 1
                amb += bool(s[gk] - s[gk - 1] <= B[p[gk]] + B[p[gk - 1]])
    return amb, tot


# ---- the cases the CPU and GPU tests share -----------------------------------------------------------------------------------------
ROUTES = [(137, 13), (22, 348), (350, 21)]      # one (group_num, group_topk) per fill route of group_select
ROW_LENGTHS = (0, 1, 63, 64, 65, 256, 257, 4096)
VOCAB = 4608


def skewed_groups(rng, n):
    """(group_of [n], ngroups): three large groups hold 45 % of the rows (the first more than 348 of 2049), the others are spread
    over up to 400 groups, so most groups are smaller than any group_topk above"""
    ng = min(400, max(1, n // 3))
    gof = rng.integers(0, ng, n)
    big = rng.permutation(n)[:(n * 45) // 100]
    gof[big] = rng.choice(min(3, ng), big.size, p=None if ng < 3 else [0.55, 0.3, 0.15])
    return gof.astype(np.uint32), ng


def _runs(rng, lengths, vocab, values):
    counts = np.asarray(lengths, np.uint32)
    idx = [np.sort(rng.choice(vocab, int(c), replace=False)).astype(np.uint32) for c in counts]
    indices = np.concatenate(idx) if idx else np.zeros(0, np.uint32)
    return counts, indices, values(indices.size).astype(np.float32)


_CASES = {}


def make_case(kind, n, nq=65):
    """(rows, queries, ref, A, m, group_of, ngroups), computed once and shared; read-only.
      "int"    integers |v| <= 6 (halves; every sum is exact in fp32): rows of ROW_LENGTHS elements, the longest on every 61st
               row; queries of 4096 / 0 / 1 / 2 / 3 pairs, the longest at 0, 17 and 64
      "zeros"  the same values, rows of 0 / 1 / 63 elements over a vocabulary of 100 000 and queries of 1 .. 3 pairs: most pairs
               share no index and score exactly 0
      "real"   Gaussian values rounded to half, rows of 20 .. 120 elements and queries of 40 over a vocabulary of 512"""
    key = (kind, n, nq)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng([77, n, nq, len(kind)])
    ints = lambda size: rng.integers(-6, 7, size)
    if kind == "int":
        rl = rng.choice(ROW_LENGTHS[:-1], n)
        rl[:min(n, 7)] = ROW_LENGTHS[:-1][:min(n, 7)]
        rl[(n - 1) % 61::61] = 4096
        ql = np.array([(0, 1, 2, 3)[q % 4] for q in range(nq)])
        ql[[q for q in (0, 17, 64) if q < nq]] = 4096
        rows, queries = _runs(rng, rl, VOCAB, ints), _runs(rng, ql, VOCAB, ints)
    elif kind == "zeros":
        rows = _runs(rng, rng.choice([0, 1, 63], n), 100000, ints)
        queries = _runs(rng, rng.choice([1, 2, 3], nq), 100000, ints)
    else:
        gauss = lambda size: rng.standard_normal(size).astype(np.float16)
        rows = _runs(rng, rng.integers(20, 121, n), 512, gauss)
        queries = _runs(rng, np.full(nq, 40), 512, gauss)
    ref, A = R.sparse_reference(rows, queries)
    m = R.shared_counts(rows, queries)
    gof, ng = skewed_groups(rng, n)
    for a in rows + queries + (ref, A, m, gof):
        a.setflags(write=False)
    _CASES[key] = (rows, queries, ref, A, m, gof, ng)
    return _CASES[key]


def take_queries(queries, which):
    """the queries numbered `which` of a (counts, indices, values) batch, as a batch"""
    c, i, v = queries
    o = R.offsets(c)
    which = list(which)
    return (np.asarray([c[q] for q in which], np.uint32),
            np.concatenate([i[o[q]:o[q + 1]] for q in which] + [np.zeros(0, np.uint32)]).astype(np.uint32),
            np.concatenate([v[o[q]:o[q + 1]] for q in which] + [np.zeros(0, np.float32)]).astype(np.float32))

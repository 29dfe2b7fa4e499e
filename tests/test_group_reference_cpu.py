"""tests/util.py group_reference and its checkers, without a GPU: on integer data (every score exact) the fp64 reference equals
oracle.flat_group_search — which other tests pin to the reference's own classes — with a filter, a radius, candidate lists and
group_topk larger than a group; and the checkers of tests/test_gpu_group_routes.py reject two deliberately broken kernel models."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util as U

N, DIM, NQ, NGROUPS = 900, 6, 7, 23


def _data(seed=3):
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, (N, DIM)).astype(np.float32)
    q = rng.integers(-3, 4, (NQ, DIM)).astype(np.float32)
    of = rng.integers(0, NGROUPS, N).astype(np.uint32)
    of[of == 5] = np.where(rng.random((of == 5).sum()) < 0.9, 6, 5)      # a small group
    of[rng.choice(N, 40, replace=False)] = NGROUPS + rng.integers(0, 5, 40).astype(np.uint32)   # rows of no group
    keys = (rng.permutation(5 * N)[:N] + 11).astype(np.uint64)
    return rng, base, q, of, keys


def _as_abi(lists, gnum, gk):
    """[(group, [(key, score)])] of one query -> the C ABI's arrays"""
    groups = np.full(gnum, U.IDX_NONE, np.uint32)
    keys = np.full((gnum, gk), ~np.uint64(0), np.uint64)
    scores = np.full((gnum, gk), np.inf, np.float32)
    counts = np.zeros(gnum, np.uint32)
    for i, (g, docs) in enumerate(lists):
        groups[i], counts[i] = g, len(docs)
        for j, (k, s) in enumerate(docs):
            keys[i, j], scores[i, j] = k, s
    return groups, len(lists), keys, scores, counts


def _oracle_abi(oracle, base, q, of, gnum, gk, m, keys, threshold, exclude, candidates):
    """oracle.flat_group_search has no group count and applies no filter to candidate lists: rows of no group are excluded,
    candidate lists are cleaned of holes and excluded rows first (their order stays)"""
    ex = (of >= NGROUPS) | (exclude if exclude is not None else False)
    cand = None if candidates is None else [[int(p) for p in c if p < N and not ex[p]] for c in candidates]
    thr = O.FLT_MAX if threshold is None else threshold
    want = oracle.flat_group_search(base, q, of, gnum, gk, m, keys=keys, threshold=thr, exclude_bits=O.pack_bits(ex), candidates=cand)
    return [_as_abi([(g, [(d[0], d[1]) for d in docs]) for g, docs in w], gnum, gk) for w in want]


@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
@pytest.mark.parametrize("gnum,gk", [(4, 5), (NGROUPS + 3, 2), (6, 200), (1, 1)])
def test_reference_equals_oracle_on_exact_data(oracle, metric, gnum, gk):
    rng, base, q, of, keys = _data()
    m = O.METRIC_L2 if metric == "SquaredEuclidean" else O.METRIC_IP
    exclude = rng.random(N) < 0.3
    all_s = U.group_reference(base, q, of, NGROUPS, gnum, gk, metric)["s64"]
    radius = float(np.sort(all_s[0])[N // 6])
    cands = [np.concatenate([rng.choice(N, int(rng.integers(1, 300)), replace=False), [U.IDX_NONE, N + 3, 17, 17]]) for _ in range(NQ)]
    cands[2] = np.zeros(0, np.int64)
    for thr, ex, cand in [(None, None, None), (radius, None, None), (None, exclude, None), (radius, exclude, cands), (None, None, cands)]:
        ref = U.group_reference(base, q, of, NGROUPS, gnum, gk, metric, threshold=thr, exclude=ex, candidates=cand)
        got = _oracle_abi(oracle, base, q, of, gnum, gk, m, keys, thr, ex, cand)
        for qi in range(NQ):
            U.check_groups_exact(ref["queries"][qi], *got[qi], gk, keys, threshold=thr, what="q%d" % qi)
            # and the reference's own lists are what the checker derives
            for g, p, s in ref["queries"][qi]["groups"]:
                assert len(p) <= gk and np.all(of[p] == g) and (thr is None or np.all(s <= thr))
        assert len(ref["queries"][2]["groups"]) == 0 or cand is None


def _model(base, q, of, gnum, gk, keys, metric, larger_ordinal=False, drop=None):
    """a kernel model built on plain sorting: the right answer, or one that keeps the LARGER ordinal of tied documents, or one
    that loses the group at place `drop`"""
    s64 = U.label_reference(base, q, metric)[0]
    out = []
    for qi in range(len(q)):
        per = {}
        for g in range(NGROUPS):
            pos = np.nonzero(of == g)[0]
            o = np.lexsort((-pos if larger_ordinal else pos, s64[qi, pos]))
            per[g] = [(keys[p], s64[qi, p]) for p in pos[o][:gk]]
        order = sorted((g for g in per if per[g]), key=lambda g: (per[g][0][1], g))
        if drop is not None:
            del order[drop]
        out.append(_as_abi([(g, per[g]) for g in order[:gnum]], gnum, gk))
    return out


@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
def test_exact_checker_rejects_broken_models(metric):
    _, base, q, of, keys = _data()
    gnum, gk = 5, 4
    ref = U.group_reference(base, q, of, NGROUPS, gnum, gk, metric)

    def run(model):
        for qi in range(NQ):
            U.check_groups_exact(ref["queries"][qi], *model[qi], gk, keys, what="q%d" % qi)
    run(_model(base, q, of, gnum, gk, keys, metric))
    with pytest.raises(AssertionError):
        run(_model(base, q, of, gnum, gk, keys, metric, larger_ordinal=True))
    for drop in (0, 2, gnum - 1):
        with pytest.raises(AssertionError):
            run(_model(base, q, of, gnum, gk, keys, metric, drop=drop))


@pytest.mark.parametrize("metric", ["SquaredEuclidean", "InnerProduct"])
def test_band_checker_on_real_data(metric):
    """the fp64 answer itself passes with no differing list; a document from far outside the band, a lost group and a score
    off by 1e-4 relative are rejected"""
    rng = np.random.default_rng(8)
    n, dim, gnum, gk, ng = 3000, 40, 6, 5, 50
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    of = (np.arange(n) % ng).astype(np.uint32)
    ref = U.group_reference(base, q, of, ng, gnum, gk, metric)
    ident = {i: i for i in range(n)}

    def answer(qi):
        return _as_abi([(g, list(zip(p.tolist(), s.astype(np.float32).tolist()))) for g, p, s in ref["queries"][qi]["groups"]], gnum, gk)

    def check(qi, a):
        return U.check_groups_band(ref, qi, *a, gnum, gk, ident, metric, dim, what="q%d" % qi)
    for qi in range(3):
        assert check(qi, answer(qi))[0] == 0 and check(qi, answer(qi))[2] == gnum and not check(qi, answer(qi))[3]
    g, k, s, c = 0, 2, 3, 4
    a = answer(0)
    grp = int(a[g][1])
    a[k][1, gk - 1] = ref["queries"][0]["order"][grp][1][-1]           # the worst member of the group
    with pytest.raises(AssertionError):
        check(0, a)
    a = answer(0)
    a[g][gnum - 1] = ref["queries"][0]["bests"][1][-1]                 # the worst group
    a[k][gnum - 1, 0] = ref["queries"][0]["order"][int(a[g][gnum - 1])][1][0]
    a[c][gnum - 1] = 1
    with pytest.raises(AssertionError):
        check(0, a)
    a = answer(0)
    a[s][0, 1] *= np.float32(1 + 1e-4)
    with pytest.raises(AssertionError):
        check(0, a)

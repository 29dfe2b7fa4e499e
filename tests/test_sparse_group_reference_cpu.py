"""tests/sparse_group_ref.py checked on the CPU: the reference against a brute-force restatement of FlatSparseEntity::search_group
(a dict of bounded heaps, one per group, filled candidate by candidate), the exact checker against five broken models, the band
checker against scores accumulated in half precision, and the ambiguity cap of the real-valued case the GPU test uses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_fp16_ref as H  # noqa: E402
import sparse_group_ref as G  # noqa: E402


def brute_force(scores, group_of, ngroups, gnum, gk, threshold=None, exclude=None, candidates=None, larger_group_first=False,
                threshold_first=False, once=False):
    """search_group restated: walk the candidates in scan order, keep per group a list of at most gk (score, ordinal, position)
    whose worst entry a strictly better candidate replaces; then rank the groups and cut at the radius.  The three flags are the
    broken models."""
    out = []
    n = scores.shape[1]
    for q in range(scores.shape[0]):
        cand = range(n) if candidates is None else [int(p) for p in candidates[q]]
        if once:
            cand = list(dict.fromkeys(cand))
        heaps = {}
        for ordinal, p in enumerate(cand):
            if p >= n or (exclude is not None and exclude[p]) or group_of[p] >= ngroups:
                continue
            s = float(scores[q, p])
            if threshold_first and threshold is not None and np.float32(s) > np.float32(threshold):
                continue
            h = heaps.setdefault(int(group_of[p]), [])
            h.append((s, ordinal, p))
            h.sort()
            del h[gk:]
        ranked = sorted(heaps, key=lambda g: (heaps[g][0][0], -g if larger_group_first else g))[:gnum]
        groups = []
        for g in ranked:
            docs = [(s, p) for s, _, p in heaps[g] if threshold is None or not np.float32(s) > np.float32(threshold)]
            groups.append((g, np.array([p for _, p in docs], np.int64), np.array([s for s, _ in docs], np.float64)))
        out.append({"groups": groups})
    return out


def _tie_case():
    """130 rows, 9 queries, integer scores in [-3, 3] (ties everywhere), 12 groups of unequal size, one row in no group"""
    rng = np.random.default_rng(5)
    n, nq = 130, 9
    scores = rng.integers(-3, 4, (nq, n)).astype(np.float64)
    group_of = rng.integers(0, 12, n).astype(np.uint32)
    group_of[7] = 12
    exclude = rng.random(n) < 0.1
    lists = [rng.integers(0, n + 20, rng.integers(0, 90)) for _ in range(nq)]
    lists[3] = np.concatenate([lists[3], lists[3][:10]])          # positions listed twice
    lists[4] = np.zeros(0, np.int64)
    return scores, group_of, 12, exclude, lists


@pytest.mark.parametrize("gnum,gk", [(3, 2), (12, 1), (5, 40), (20, 7)])
@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("threshold", [None, -1.0])
def test_reference_equals_the_brute_force(gnum, gk, listed, threshold):
    scores, gof, ng, exclude, lists = _tie_case()
    cand = lists if listed else None
    key_of = np.arange(scores.shape[1], dtype=np.uint64) + np.uint64(1000)
    want = G.render(brute_force(scores, gof, ng, gnum, gk, threshold, exclude, cand), gnum, gk, key_of)
    got = G.render(G.select(scores, gof, ng, gnum, gk, threshold, exclude, cand), gnum, gk, key_of)
    G.check_exact(want, got)
    G.check_exact(got, want)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)


def test_reference_on_sparse_integer_rows():
    """the same on real sparse rows: the "int" case, scores from sparse_reference"""
    rows, queries, ref, A, m, gof, ng = G.make_case("int", 129)
    assert np.all(ref == np.round(ref)) and np.abs(ref).max() < 2 ** 24
    key_of = np.arange(129, dtype=np.uint64)
    for gnum, gk in ((5, 3), (43, 50)):
        r = G.group_reference((rows, queries, ref, A, m), gof, ng, gnum, gk)
        G.check_exact(G.render(brute_force(ref, gof, ng, gnum, gk), gnum, gk, key_of), G.render(r["queries"], gnum, gk, key_of))


def _rejects(want, got):
    with pytest.raises(AssertionError):
        G.check_exact(want, got)


def test_exact_checker_rejects_the_broken_models():
    scores, gof, ng, exclude, lists = _tie_case()
    gnum, gk, thr = 5, 4, -1.0
    key_of = np.arange(scores.shape[1], dtype=np.uint64)
    want = G.render(G.select(scores, gof, ng, gnum, gk, thr, exclude, lists), gnum, gk, key_of)
    G.check_exact(want, tuple(a.copy() for a in want))
    # a dropped document: the last one of a list that has two
    q, i = np.argwhere(want[4] >= 2)[0]
    got = tuple(a.copy() for a in want)
    got[4][q, i] -= 1
    _rejects(want, got)
    # a swapped tie: two neighbours of equal score change places
    got = tuple(a.copy() for a in want)
    done = False
    for q, i in np.argwhere(want[4] >= 2):
        for j in range(int(want[4][q, i]) - 1):
            if want[3][q, i, j] == want[3][q, i, j + 1] and want[2][q, i, j] != want[2][q, i, j + 1]:
                got[2][q, i, [j, j + 1]] = got[2][q, i, [j + 1, j]]
                done = True
                break
        if done:
            break
    assert done
    _rejects(want, got)
    # the three models of brute_force
    for flag in ("larger_group_first", "threshold_first", "once"):
        broken = G.render(brute_force(scores, gof, ng, gnum, gk, thr, exclude, lists, **{flag: True}), gnum, gk, key_of)
        _rejects(want, broken)


REAL_N = 2049


def test_band_checker_and_the_ambiguity_cap_of_the_real_case():
    rows, queries, ref, A, m, gof, ng = G.make_case("real", REAL_N, 4)
    assert ng >= 350 and np.bincount(gof).max() > 348
    pos_of_key = {p: p for p in range(REAL_N)}
    key_of = np.arange(REAL_N, dtype=np.uint64)
    half = H.half_accumulated_scores(rows, queries).astype(np.float64)
    s32 = ref.astype(np.float32).astype(np.float64)                 # the reference rounded once: inside every band
    for gnum, gk in G.ROUTES:
        r = G.group_reference((rows, queries, ref, A, m), gof, ng, gnum, gk)
        amb, tot = G.ambiguity(r, gnum, gk)
        assert tot > 0 and amb * 4 <= tot, (gnum, gk, amb, tot)
        good = G.render(G.select(s32, gof, ng, gnum, gk), gnum, gk, key_of)
        bad = G.render(G.select(half, gof, ng, gnum, gk), gnum, gk, key_of)
        for q in range(len(queries[0])):
            G.check_band(r, q, good[0][q], good[1][q], good[2][q], good[3][q], good[4][q], gnum, gk, pos_of_key)
        with pytest.raises(AssertionError):
            for q in range(len(queries[0])):
                G.check_band(r, q, bad[0][q], bad[1][q], bad[2][q], bad[3][q], bad[4][q], gnum, gk, pos_of_key)

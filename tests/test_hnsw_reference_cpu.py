"""The HNSW search model and its fixtures (tests/hnsw_ref.py) on the CPU: the model against brute force and against answers written
out by hand, and every fixture of tests/test_gpu_hnsw.py against the precondition it is there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_ref as H  # noqa: E402


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_model_is_exact_at_full_width(metric):
    """ef = n, max_scan = n on a connected graph: the exact top-k of brute force"""
    g = H.exact_graph(300, 20, 4)
    n = g.rows.shape[0]
    assert len(H.reachable(g)) == n
    rng = np.random.default_rng(1)
    for q in H.exact_queries(g, rng, 6):
        res = H.search_model(g, q, 10, n, n, metric=metric)
        keys, scores = H.brute_force(g, q, 10, metric)
        assert np.array_equal(res.keys, keys) and np.array_equal(res.scores, scores)
        assert res.scanned == res.dists.size >= n          # (every row once on level 0, some again on the upper levels)


def test_hand_made_answers():
    q = lambda x: np.array([x, 0, 0, 0], np.float32)    # noqa: E731
    # chain: the walk goes 0, 1, 2, ... while the nearest candidate is no farther than the worst result
    r = H.search_model(H.chain(), q(10.2), 3, 3)
    assert r.keys.tolist() == [10, 11, 9] and r.hops == 12 and r.scanned == 13
    # ... and ef = 1 stops at the first node that is not an improvement: node 10 is expanded, node 11 is farther than node 10
    r = H.search_model(H.chain(), q(10.2), 1, 1)
    assert r.keys.tolist() == [10] and r.hops == 11 and r.scanned == 12
    # star: one expansion computes all 69 leaves, and with that every row: the walk ends on max_scan = n
    r = H.search_model(H.star(), q(30.4), 2, 2)
    assert r.keys.tolist() == [30, 31] and r.scanned == 70 and r.hops == 1 and r.on_limit
    # two components: the answer is the entry point's component, however near the other one is
    r = H.search_model(H.two_components(), q(12.0), 20, 20)
    assert r.keys.tolist() == [4, 3, 2, 1, 0] and r.scanned == 5 and r.hops == 5
    # empty lists: 3 and 6 are reached and returned, expanding them finds nothing; 0, 1, 2, 3, 4, 5, 6 and 7 are expanded, then
    # every row has been computed
    r = H.search_model(H.with_empty_lists(), q(0.0), 10, 10)
    assert r.keys.tolist() == list(range(10)) and r.scanned == 10 and r.hops == 8
    # upper levels: level 2 moves 0 -> 9 (distance 1 to the query at 8), 9 has no list there or on level 1; on level 0 node 9 is
    # expanded (8 and 10 computed), then 8 (7 computed, 9 visited), and nothing nearer than 8 is left
    r = H.search_model(H.bare_upper(), q(8.0), 1, 1)
    assert r.keys.tolist() == [8] and r.scanned == 1 + 1 + 2 + 1 and r.hops == 2
    # n = 1
    r = H.search_model(H.single(), q(5.0), 4, 4)
    assert r.keys.tolist() == [0] and r.scores.tolist() == [25.0] and r.scanned == 1 and r.hops == 0
    # duplicates count once
    r = H.search_model(H.duplicate_ids(), q(0.0), 8, 8)
    assert r.keys.tolist() == [0, 2, 1, 3, 4, 5, 6, 7] and r.scanned == 8 and r.hops == 3
    # ties: ascending node id inside one distance
    r = H.search_model(H.tie_ring(), q(0.0), 8, 64)
    assert r.keys.tolist() == [0, 16, 32, 48, 1, 17, 33, 49] and r.scores.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("name", list(H.HAND_MADE))
def test_hand_made_graphs_are_valid(name):
    H.check_graph(H.HAND_MADE[name]())


def test_fixture_preconditions():
    for dim, m in [(4, 4), (20, 8), (100, 4), (128, 8)]:
        g = H.exact_graph(1500, dim, m)
        H.check_graph(g)
        assert g.max_level >= 1 and g.m0 == 2 * m and len(H.reachable(g)) == 1500
    g = H.exact_graph(1500, 20, 8)
    rng = np.random.default_rng(2)
    q = H.exact_queries(g, rng, 8)
    # the tie fixtures really contain ties: equal distances among what one walk computes
    for x in q:
        d = H.search_model(g, x, 10, 64).dists
        assert np.unique(d).size < d.size
    d = H.search_model(H.tie_ring(), np.zeros(4, np.float32), 8, 64).dists
    assert np.unique(d).size * 4 <= d.size
    # the scan-limit fixture really stops on the limit, also inside the upper levels' count
    full = H.search_model(g, q[0], 10, 64)
    for ms in (1, 2, 40, full.scanned // 2):
        r = H.search_model(g, q[0], 10, 64, max_scan=ms)
        assert r.on_limit and r.scanned >= ms and r.scanned < full.scanned
    upper_only = H.search_model(g, q[0], 10, 64, max_scan=2)
    assert upper_only.scanned > 2 and upper_only.hops == 0          # (the upper levels alone pass the limit: no expansion)
    # the candidate-capacity fixtures really overflow C: its capacity is max_scan, and one expansion brings more than that
    assert H.search_model(H.star(), np.array([30, 0, 0, 0], np.float32), 5, 5, max_scan=10).evicted > 0
    assert H.search_model(H.tie_ring(), np.zeros(4, np.float32), 8, 64, max_scan=3).evicted == 1
    # excluding a neighbourhood lets C grow past ef, excluding everything past what the kernel keeps in LDS
    ex = np.zeros(1500, bool)
    ex[[int(k - 3) // 7 for k in H.search_model(g, q[0], 200, 200).keys]] = True
    r = H.search_model(g, q[0], 10, 10, exclude=ex)
    assert r.c_peak > 10 and not set(r.keys.tolist()) & set((np.nonzero(ex)[0] * 7 + 3).tolist())
    r = H.search_model(g, q[0], 10, 10, exclude=np.ones(1500, bool))
    assert r.keys.size == 0 and r.c_peak > 512 and r.scanned >= 1500
    big = H.exact_graph(3000, 20, 8)
    r = H.search_model(big, q[0], 10, 10, exclude=np.ones(3000, bool))
    assert r.c_peak > H.C_LDS and r.hops > r.c_peak                 # (candidates are popped after the set has left LDS)
    r = H.search_model(H.star(1200), np.zeros(4, np.float32), 10, 10, exclude=np.ones(1200, bool))
    assert r.c_peak > H.C_LDS


@pytest.mark.parametrize("dim", sorted(H.REAL))
def test_real_fixture_is_mostly_decisive(dim):
    g, q = H.real_graph(dim)
    H.check_graph(g)
    good = 0
    for x in q:
        res = H.search_model(g, x, H.REAL_TOPK, H.REAL_EF)
        good += H.decisive(res, H.band(g, x, res.nodes))
    assert good * 4 >= 3 * len(q), (good, len(q))

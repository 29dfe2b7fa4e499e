"""The model and fixtures of tests/hnsw_build_ref.py held to their preconditions: every fixture is a valid graph and shows what it is
for, the round model with one node per round is a plain sequential insertion, the level generator is the published SplitMix64 and
has the distribution it claims, and the recorded recall of the sequential model is the one it has."""
import bisect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402


@pytest.mark.parametrize("name", list(B.FIXTURES))
def test_fixture_is_a_valid_graph(name):
    fx, g, c, book = B.model_of(name)
    n = fx.rows.shape[0]
    H.check_graph(g)
    p = fx.params
    assert (g.m0, g.m) == (p.m0, p.m) and g.max_level == int(fx.levels.max())
    assert sum(book["round_sizes"]) == n - 1 and c.rounds == len(book["round_sizes"])
    assert c.requests >= c.prunes and (c.prunes > 0 or c.requests * 2 == int(g.cnt0.sum()) + int(g.cnt_up.sum()))
    for v in range(n):                                  # no self-link, no repeat
        x = g.nbr0[v, :g.cnt0[v]]
        assert v not in x and len(set(x.tolist())) == x.size
    if name not in ("duplicates", "line_clusters"):     # (distance 0 between distinct nodes lets the keep rule cut whole groups off)
        assert len(H.reachable(g)) >= (n * 9) // 10


def _sequential(rows, p, levels, metric):
    """add_node, update_neighbors and reverse_update_neighbors one node at a time, written without the round machinery"""
    n = rows.shape[0]
    D = B.distance_matrix(rows, metric)
    lists = [[[] for _ in range(n)] for _ in range(int(levels.max()) + 1)]

    def keep(cands, cap):
        out = []
        for d, c in cands:
            if not any(D[c, s] <= d for s in out):
                out.append(c)
                if len(out) == cap:
                    break
        return out

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
        found = {}
        for level in range(min(li, top), -1, -1):
            seen, R, Cq = {ep}, [(D[i, ep], ep)], [(D[i, ep], ep)]
            while Cq:
                dc, c = Cq[0]
                if len(R) == p.ef_construction and dc > R[-1][0]:
                    break
                Cq.pop(0)
                for v in [v for v in lists[level][c] if v not in seen]:
                    seen.add(v)
                    if len(R) < p.ef_construction or D[i, v] < R[-1][0]:
                        bisect.insort(Cq, (D[i, v], v))
                        bisect.insort(R, (D[i, v], v))
                        del R[p.ef_construction:]
            found[level] = R
            ep = R[0][1]
        for level, W in found.items():
            cap = p.m0 if level == 0 else p.m
            if len(W) <= min(p.prune_cnt, cap):
                sel = [v for _, v in W]
            else:
                sel = keep(W, cap)
                sel += [v for _, v in W if v not in sel][:max(0, p.min_neighbors - len(sel))]
            lists[level][i] = list(sel)
            for t in sel:
                if len(lists[level][t]) < cap:
                    lists[level][t].append(i)
                else:
                    lists[level][t] = keep(sorted((D[t, x], x) for x in lists[level][t] + [i]), cap)
        if li > top:
            entry, top = i, li
    return lists, entry


@pytest.mark.parametrize("name", ["l2-div0-max7", "ip-div0-max64", "min_neighbors", "duplicates"])
def test_one_node_per_round_is_sequential_insertion(name):
    fx, _, _, _ = B.model_of(name)
    g, c = B.build_model(fx.rows, fx.params, fx.levels, 0, fx.round_max, fx.metric)
    lists, entry = _sequential(fx.rows, fx.params, fx.levels, fx.metric)
    assert g.entry_point == entry and c.rounds == fx.rows.shape[0] - 1
    for v in range(fx.rows.shape[0]):
        assert g.nbr0[v, :g.cnt0[v]].tolist() == lists[0][v]
        for l in range(1, int(fx.levels[v]) + 1):
            u = g.upper_of[v]
            assert g.nbr_up[u, l - 1, :g.cnt_up[u, l - 1]].tolist() == lists[l][v]


def test_fixtures_show_what_they_are_for():
    for name in B.FIXTURES:
        fx, g, c, book = B.model_of(name)
        if fx.rows.shape[0] >= 300:
            assert book["dropped_links"] > 0, name                         # some prune drops a link the target had
            assert 0 < book["shortcuts"], name                             # some W is taken whole
            assert book["own_rounds"] == 2 or name == "sliced", name       # the level-2 and level-3 nodes mid-sequence
    for name in ("l2-div1-max64", "ip-div1-max64", "line_clusters", "sliced"):
        book = B.model_of(name)[3]
        assert book["max_requests"] > book["max_requests_cap"], name       # more requests to one target in a round than it holds
    assert B.model_of("all_shortcut")[3]["shortcuts"] == B.model_of("all_shortcut")[3]["selections"]
    assert B.model_of("l2-div16-max64")[3]["shortcuts"] < B.model_of("l2-div16-max64")[3]["selections"]
    assert B.model_of("min_neighbors")[3]["filled"] > 0 and B.model_of("l2-div16-max64")[3]["filled"] == 0
    assert B.model_of("prune_cnt_small")[3]["shortcuts"] < B.model_of("l2-div16-max64")[3]["shortcuts"] \
        < B.model_of("prune_cnt_large")[3]["shortcuts"]
    assert max(B.model_of("wide")[1].cnt0) > 64                            # a list wider than a wave
    assert max(B.model_of("l2-div1-max7")[3]["round_sizes"]) == 7 and max(B.model_of("l2-div1-max64")[3]["round_sizes"]) == 64
    assert B.model_of("n35")[3]["round_sizes"][-3:] == [1, 2, 1]           # one node past the first round of two
    fx = B.sliced()
    assert (B.slices_of(fx, 1 << 30), B.slices_of(fx, 6400), B.slices_of(fx, 1024)) == (1, 3, 17)
    rows = B.duplicates().rows
    assert np.unique(rows, axis=0).shape[0] <= 40


def test_rounds():
    lv = np.zeros(100, np.uint32)
    assert [(s, e) for s, e, _, _ in B.rounds_of(lv, 0, 64)] == [(i, i + 1) for i in range(1, 100)]
    assert [(s, e) for s, e, _, _ in B.rounds_of(lv, 1, 16)] == [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32), (32, 48), (48, 64), (64, 80),
                                                                 (80, 96), (96, 100)]
    lv[5] = 2                                           # ends the round [4, 8) before it, is a round of its own, becomes the entry
    lv[6] = 1
    plan = B.rounds_of(lv, 1, 16)
    assert plan[:5] == [(1, 2, 0, 0), (2, 4, 0, 0), (4, 5, 0, 0), (5, 6, 0, 0), (6, 12, 5, 2)]


def test_levels_model():
    # the published first outputs of SplitMix64 from state 0
    assert [B.splitmix64((i * B.GOLD) & B.M64) for i in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    by_hand = []
    for i in range(200):
        r = B.splitmix64((11 + i * B.GOLD) & B.M64) >> 11
        by_hand.append(min(sum(1 for k in range(1, 60) if r * 5 ** k < 2 ** 53), B.MAX_LEVEL))
    assert B.levels_model(200, 5, 11).tolist() == by_hand
    assert B.level_thresholds(1000)[-1] == 1 and B.level_thresholds(5)[0] == -(-2 ** 53 // 5)
    for sf in (5, 16):
        lv = B.levels_model(10 ** 6, sf, 3)
        for k in (1, 2, 3):                             # P(level >= k) = sf^-k, within five standard deviations
            pk = float(sf) ** -k
            assert abs((lv >= k).mean() - pk) < 5 * (pk * (1 - pk) / 1e6) ** 0.5
    assert B.levels_model(10 ** 6, 5, 3).max() <= B.MAX_LEVEL


def test_quality_constant():
    rows, q, levels = B.quality_data()
    g, _ = B.build_model(rows, B.QUALITY_PARAMS, levels, 0, 1)
    H.check_graph(g)
    found = [H.search_model(g, x, B.QUALITY_K, B.QUALITY_EF).keys for x in q]
    assert abs(B.recall(found, B.quality_truth(rows, q)) - B.QUALITY_P) < 1e-9
    assert 0.011 < B.QUALITY_P - B.quality_floor() < 0.012

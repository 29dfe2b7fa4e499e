"""The model of appending to an HNSW graph (tests/hnsw_add_ref.py) held to its preconditions without a GPU: with no call boundary it
is the build's model; the consequences P1 and P2 of DESIGN §3c "Appending" hold in it; every fixture shows what it is there for,
read from the model's own bookkeeping."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_add_ref as A  # noqa: E402
import hnsw_build_ref as B  # noqa: E402
import hnsw_ref as H  # noqa: E402


def _same_graph(g, r):
    assert np.array_equal(g.rows, r.rows) and np.array_equal(g.keys, r.keys)
    assert (g.m0, g.max_level, g.m, g.n_upper, g.entry_point) == (r.m0, r.max_level, r.m, r.n_upper, r.entry_point)
    for a, b in ((g.nbr0, r.nbr0), (g.cnt0, r.cnt0), (g.upper_of, r.upper_of), (g.nbr_up, r.nbr_up), (g.cnt_up, r.cnt_up)):
        assert np.array_equal(a, b)


def _total(calls):
    return B.Counters(*[sum(c.counters[k] for c in calls) for k in range(4)])


@pytest.mark.parametrize("name", list(B.FIXTURES))
def test_without_a_boundary_it_is_the_build_model(name):
    fx, g, c, _ = B.model_of(name)
    n = fx.rows.shape[0]
    calls = A.add_model(fx.rows, fx.params, fx.levels, (n,), fx.round_div, fx.round_max, fx.metric)
    assert len(calls) == 1 and calls[0].counters == c
    _same_graph(calls[0].graph, g)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_p1_sequential_rounds_do_not_see_the_cuts(metric):
    fx = B.base(metric, 0, 64)
    g, c = B.build_model(fx.rows, fx.params, fx.levels, 0, 64, metric)
    calls = A.add_model(fx.rows, fx.params, fx.levels, (100, 1, 7, 64, 428), 0, 64, metric)
    _same_graph(calls[-1].graph, g)
    assert _total(calls) == c
    assert all(k.book["one_rounds"] == k.counters.rounds for k in calls)


def test_p2_one_row_per_call_is_the_sequential_graph():
    fx = B.base("l2", 16, 64)
    n = 150
    g, c = B.build_model(fx.rows[:n], fx.params, fx.levels[:n], 0, 64, "l2")
    calls = A.add_model(fx.rows[:n], fx.params, fx.levels[:n], (1,) * n, 16, 64, "l2")
    _same_graph(calls[-1].graph, g)
    assert _total(calls) == c
    # and with rounds of more than one node the cut graph is NOT the uncut one: the boundary is visible, as the rule says
    whole = B.build_model(fx.rows, fx.params, fx.levels, 16, 64, "l2")[0]
    assert not np.array_equal(A.model_of("cut")[1][-1].graph.nbr0, whole.nbr0)


def test_cut_falls_inside_rounds():
    fx, calls = A.model_of("cut")
    whole = B.rounds_of(fx.levels, fx.round_div, fx.round_max)
    assert fx.levels[200] == 2                           # (the first add begins with a node that is a round of its own either way)
    for k in calls[2:]:
        inside = [r for r in whole if r[0] < k.first < r[1]]
        assert len(inside) == 1, k.first                 # one build would have carried a round across this boundary
    assert [k.count for k in calls] == [200, 37, 1, 150, 212]
    assert calls[2].book["round_sizes"] == [1]
    assert max(calls[1].book["round_sizes"]) > 1 and max(calls[4].book["round_sizes"]) > 1
    for g in (c.graph for c in calls):
        H.check_graph(g)


def test_top_raised_restrides_inside_and_at_the_head_of_a_call():
    fx, calls = A.model_of("top_raised")
    assert [k.graph.max_level for k in calls] == [1, 3, 3]
    assert [k.restrided for k in calls] == [True, True, False]          # (the build makes the table; the third call fits it)
    assert calls[1].book["own_rounds"] == [50] and 0 < 50 < calls[1].count - 1
    assert fx.levels[calls[2].first] == 2 and calls[2].book["own_rounds"] == []
    assert calls[1].graph.entry_point == 200 and calls[2].graph.entry_point == 200
    assert calls[0].graph.n_upper >= 10                                 # a table worth moving
    assert calls[1].graph.cnt_up[:, 1:].sum() == 0 and calls[2].graph.cnt_up[:, 1].sum() == 2      # 250 <-> 200 on level 2


def test_first_upper_makes_the_upper_arrays_in_an_add():
    fx, calls = A.model_of("first_upper")
    assert calls[0].graph.max_level == 0 and not calls[0].restrided
    assert calls[1].graph.max_level == 2 and calls[1].restrided and calls[1].graph.n_upper == 3
    assert calls[1].book["own_rounds"] == [20, 40]
    assert calls[2].graph.n_upper == 4 and not calls[2].restrided
    assert calls[2].graph.upper_of[170] == 3 and calls[2].graph.cnt_up[3, 0] > 0


def test_prune_old_drops_links_from_before_the_call():
    fx, calls = A.model_of("prune_old")
    assert calls[1].book["dropped_old_links"] >= 1 and calls[1].counters.prunes >= 1


def test_wide_lists_on_both_paths():
    fx, calls = A.model_of("wide")
    assert fx.params.m0 > 64
    assert max(calls[1].book["round_sizes"]) > 1 and int(calls[1].graph.cnt0.max()) > 64
    assert all(k.count == 1 and k.book["round_sizes"] == [1] for k in calls[2:]) and len(calls) == 12
    assert sum(k.book["long_one"] for k in calls[2:]) >= 1              # a round of one node appends behind the 64th id of a list


def test_spill_begins_past_the_lds_candidates():
    fx, calls = A.model_of("spill")
    assert calls[1].first > H.C_LDS and calls[1].book["round_sizes"] == [34, 34, 2]
    assert A.slices_of(fx, 1, 1 << 30) == 1 and A.slices_of(fx, 1, 103776) == 3 and A.slices_of(fx, 1, 17296) == 17


def test_ip_is_cut_under_inner_product():
    fx, calls = A.model_of("ip")
    l2 = A.model_of("cut")[0]
    assert fx.metric == "ip" and fx.calls == l2.calls and np.array_equal(fx.rows, l2.rows)
    assert not np.array_equal(calls[-1].graph.nbr0, A.model_of("cut")[1][-1].graph.nbr0)


def test_some_prune_happens_on_the_one_node_path():
    """the one-node reverse kernel has to prune somewhere: P1's calls and `wide`'s call of one row"""
    calls = A.add_model(B.base().rows, B.base().params, B.base().levels, (100, 1, 7, 64, 428), 0, 64, "l2")
    assert sum(k.book["prunes_one"] for k in calls[1:]) > 0

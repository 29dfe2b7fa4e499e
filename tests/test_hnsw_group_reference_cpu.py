"""The fp64 model of the group-by HNSW search (tests/hnsw_group_ref.py) against brute force, and the facts its fixtures exist for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hnsw_group_ref as G  # noqa: E402
import hnsw_ref as H  # noqa: E402


@pytest.mark.parametrize("gnum,gk,metric", [(3, 2, "l2"), (7, 4, "l2"), (5, 3, "ip")])
def test_whole_walk_equals_brute_force(gnum, gk, metric):
    """a connected graph walked with ef = n and no scan limit: R is every admitted node, so grouping it is grouping the index"""
    g = H.exact_graph(600, 16, 8)
    n = g.rows.shape[0]
    assert len(H.reachable(g)) == n
    group_of = np.where(np.arange(n) % 11 == 0, G.NONE, np.arange(n) % 7).astype(np.uint32)
    exclude = np.arange(n) % 4 == 2
    for q in H.exact_queries(g, np.random.default_rng(9), 4):
        m = G.group_search_model(g, q, group_of, 7, gnum, gk, n, exclude=exclude, metric=metric)
        b = G.brute_force_grouped(g, q, group_of, 7, gnum, gk, exclude, metric)
        assert not m.expanded and m.groups == b.groups and len(m.groups) == gnum
        assert [x.tobytes() for x in m.keys + m.scores] == [y.tobytes() for y in b.keys + b.scores]


@pytest.mark.parametrize("name", list(G.cases()))
def test_fixture_shows_its_fact(name):
    c = G.cases()[name]
    ms = G.model_of(c)
    assert c.fact(ms)
    for m in ms:                                     # no excluded or group-less node is ever listed
        nodes = np.searchsorted(c.g.keys, np.concatenate([np.zeros(0, np.uint64)] + m.keys))
        assert (c.group_of[nodes] < c.ngroups).all() and (c.exclude is None or not c.exclude[nodes].any())

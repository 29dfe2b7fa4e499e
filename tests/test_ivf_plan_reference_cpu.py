"""The fixtures of tests/test_gpu_ivf_plan.py held to their preconditions, without a GPU (tests/ivf_plan_ref.py).

A fixture that stops doing what it is there for — a probe count that no longer sits on a pass boundary, a scan that fits one round,
a batch without a 17-row last group — fails here instead of passing on the GPU.  And for every carry of the plan the restatement is
run with that carry forgotten: the answer must change, which is how "the GPU test would fail on such a kernel" is shown without
touching a kernel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_plan_ref as P  # noqa: E402


def _untied(fx, nprobe):
    probe, d = P.coarse_ranking(fx["cent"], fx["queries"], nprobe)
    upto = min(nprobe + 1, fx["nlist"])
    assert (np.diff(d[:, :upto], axis=1) > 0).all(), "%s: tied coarse ranking" % fx["name"]
    # ... and far from tied: exact in fp32 and fp16, whatever order the sums are taken in
    assert np.diff(d[:, :upto], axis=1).min() >= 2.0
    return probe


def _answer(fx, pl, k, excluded=None):
    return P.topk_reference(pl["probed"], fx["sizes"], fx["vecs"], fx["queries"], k, excluded)


def _plan(fx, nprobe, max_scan, tpc=2, nt=1024, drop=None, brute_force=False):
    probe = _untied(fx, nprobe)
    ltpc = P.level_tpc(P.list_levels(fx["sizes"]), tpc)
    return P.plan(probe, fx["sizes"], max_scan, ltpc, nt=nt, drop=drop, brute_force=brute_force)


def test_level_and_chunk_restatements():
    """level_tpc and the three levels on hand-checked cases"""
    assert list(P.level_tpc([0, 1, 2], 2)) == [4, 2, 1] and list(P.level_tpc([0, 1, 2], 8)) == [16, 8, 2]
    assert list(P.level_tpc([0, 1, 2], 32)) == [32, 32, 8] and list(P.level_tpc([0, 1, 2], 1)) == [2, 1, 1]
    # 200 one-tile lists: the first half of the deal order is the head, the last quarter the tail
    lv = P.list_levels(np.full(200, 30))
    assert (lv[:100] == 0).all() and (lv[100:150] == 1).all() and (lv[150:] == 2).all()
    assert list(P.chunks_of([1, 128, 129, 1153], np.array([1, 1, 1, 4]))) == [1, 1, 2, 3]
    assert list(P.block_scan([1, 2, 3, 4, 5], 2)) == [0, 1, 3, 6, 10, 15]
    assert list(P.block_scan([1, 2, 3, 4, 5], 2, drop="scan_carry")) == [0, 1, 0, 3, 0, 5]


@pytest.mark.parametrize("nq", (4, 40))
def test_p_ranks_equal_sizes_sit_on_the_pass_boundaries(nq):
    fx = P.p_ranks("equal", nq)
    assert fx["nlist"] == 200 and (fx["sizes"] == 30).all() and fx["vecs"].shape[0] == 6000 <= 10000
    assert len({tuple(q) for q in fx["queries"]}) == nq
    for nprobe, max_scan in P.P_RANKS_PAIRS:
        pl = _plan(fx, nprobe, max_scan)
        want = P.P_RANKS_PROBED[(nprobe, max_scan)]
        assert (pl["q_nprobe"] == want).all() and (pl["q_scanned"] == 30 * want).all()
    assert sorted(P.P_RANKS_PROBED.values()) == [64, 65, 128, 129, 200]          # one, two (+1), two, three (+1) and four passes
    assert P.expected_route(4, 10, 150, fx["sizes"]) == P.ROUTE_DIRECT_BLOCK_TOPK
    assert P.expected_route(4, 100, 150, fx["sizes"]) == P.ROUTE_DIRECT_SELECT
    assert P.expected_route(40, 10, 150, fx["sizes"]) == P.ROUTE_TILE and P.expected_route(40, 500, 150, fx["sizes"]) == P.ROUTE_LARGE_K
    assert P.expected_route(4, 10, 200, fx["sizes"], brute_force=True) == P.ROUTE_TILE


def test_p_ranks_unequal_sizes_cut_every_query_elsewhere():
    fx = P.p_ranks("unequal", 40)
    assert fx["sizes"].min() == 1 and fx["sizes"].max() == 59 and fx["vecs"].shape[0] <= 10000
    for nprobe, max_scan in P.P_RANKS_PAIRS[:4]:
        pl = _plan(fx, nprobe, max_scan)
        assert len(set(pl["q_nprobe"].tolist())) >= 3, "the cut does not move with the query"
        assert (pl["q_nprobe"] < nprobe).all() and (pl["q_scanned"] >= max_scan).all()
    pl = _plan(fx, 150, 3841)
    assert pl["q_nprobe"].min() > 64 and pl["q_nprobe"].max() > 128             # two and three passes in one batch


@pytest.mark.parametrize("sizes", ("equal", "unequal"))
@pytest.mark.parametrize("nq", (4, 40))
def test_p_ranks_a_forgotten_carry_changes_the_answer(sizes, nq):
    """scanned_before / before_g forgotten: ranks past the cut are probed; slot_carry forgotten: the slots of the second pass fall on
    those of the first.  Both change the plan arrays and, through them, the top-k of most queries."""
    fx = P.p_ranks(sizes, nq)
    k = 10
    for nprobe, max_scan in P.P_RANKS_PAIRS[1:]:                                 # (64 probes: one pass, no carry in use)
        good = _plan(fx, nprobe, max_scan)
        truth = _answer(fx, good, k)
        assert P.same_answer(P.simulate_scan(good, fx["sizes"], fx["vecs"], fx["queries"], k), truth)
        if nprobe < 200:                                                         # (every list probed: nothing more to admit)
            bad = _plan(fx, nprobe, max_scan, drop="scanned_before")
            assert not np.array_equal(bad["q_nprobe"], good["q_nprobe"]) and not np.array_equal(bad["q_scanned"], good["q_scanned"])
            assert not P.same_answer(_answer(fx, bad, k), truth)
        bad = _plan(fx, nprobe, max_scan, drop="slot_carry")
        assert not np.array_equal(bad["q_nslots"], good["q_nslots"]) and bad["csr"] != good["csr"]
        if nq > P.DIRECT_MAX_Q:                                                  # (slots exist on the tile route only)
            assert not P.same_answer(P.simulate_scan(bad, fx["sizes"], fx["vecs"], fx["queries"], k), truth)


def test_p_rounds_takes_several_rounds_in_both_thread_forms():
    fx = P.p_rounds()
    nlist, nq = fx["nlist"], len(fx["queries"])
    assert (nlist, nq) == (1064, 1061) and fx["vecs"].shape[0] <= 10000
    assert fx["sizes"][fx["sizes"] > 0].min() == 3 and fx["sizes"].max() == 9
    for nt, rounds in ((1024, 2), (256, 5)):
        assert -(-nlist // nt) == rounds and -(-nq // nt) == rounds
    assert np.array_equal(P.list_order(fx["sizes"]), np.arange(nlist))           # a list's place in item_off is its id
    assert len({tuple(q) for q in fx["queries"]}) == nq
    pl = _plan(fx, P.P_ROUNDS_NPROBE, 0xffffffff)
    assert (pl["q_nprobe"] == 3).all()
    items = np.diff(pl["item_off"])
    for l in P.P_ROUNDS_UNPROBED:
        assert pl["list_count"][l] == 0 and items[l] == 0
    for l in P.P_ROUNDS_EMPTY:
        assert fx["sizes"][l] == 0 and items[l] == 0
    assert pl["list_count"][1062] == 0 and 1062 in pl["probed"][int(np.argmax(fx["queries"][:, 0]))]   # probed, yet no rows to plan
    assert (items[[254, 257, 1022, 1025]] > 0).all()                             # runs of zero-item lists across 255 | 256 and 1023 | 1024
    assert pl["total_items"] > 1024                                              # the scan's item search runs over more than 1024 entries
    # the plan does not depend on the thread form
    p256 = _plan(fx, P.P_ROUNDS_NPROBE, 0xffffffff, nt=256)
    for name in ("slot_begin", "list_qoff", "item_off"):
        assert np.array_equal(pl[name], p256[name])


@pytest.mark.parametrize("nt", (1024, 256))
def test_p_rounds_a_forgotten_scan_carry_changes_the_answer(nt):
    fx = P.p_rounds()
    k = 5
    good = _plan(fx, P.P_ROUNDS_NPROBE, 0xffffffff, nt=nt)
    truth = _answer(fx, good, k)
    assert P.same_answer(P.simulate_scan(good, fx["sizes"], fx["vecs"], fx["queries"], k), truth)
    bad = _plan(fx, P.P_ROUNDS_NPROBE, 0xffffffff, nt=nt, drop="scan_carry")
    for name in ("slot_begin", "list_qoff", "item_off"):
        assert not np.array_equal(bad[name], good[name]), name
    assert bad["total_items"] < good["total_items"]
    assert not P.same_answer(P.simulate_scan(bad, fx["sizes"], fx["vecs"], fx["queries"], k), truth)
    # queries on the two sides of a round boundary have different answers: one answered with the other's slots cannot pass
    for b in range(nt, len(fx["queries"]), nt):
        assert not np.array_equal(truth[1][b - 1], truth[1][b]) and not np.array_equal(truth[1][b - nt], truth[1][b])


def test_p_groups_covers_every_group_shape_and_level():
    last = {nq: P.group_shapes(nq) for nq in P.P_GROUPS_BATCHES}
    assert {r for _, r in last.values()} == {1, 16, 17, 32}                      # both sides of the half switch, a lone row, a full group
    assert {g for g, _ in last.values()} == {1, 2, 3, 4}                         # every within % ngroups for up to four groups
    sizes = np.asarray(P.P_GROUPS_SIZES)
    assert {1, 127, 128, 129, 9 * 128 + 1} <= set(sizes.tolist()) and sizes.sum() <= 10000
    lv = P.list_levels(sizes)
    assert set(lv.tolist()) == {0, 1, 2} and lv[int(np.argmax(sizes))] == 0
    # (an index this small is searched with a base chunk length of 2 tiles, the least the host picks; the GPU test takes it from
    # the read-back and asserts the same two properties there)
    ltpc = P.level_tpc(lv, 2)
    assert P.chunks_of(sizes, ltpc)[int(np.argmax(sizes))] == 3 and len(set(ltpc.tolist())) == 3
    assert len(set(P.chunks_of(sizes, ltpc).tolist())) >= 3                      # 1, 2 and 3 chunks
    assert not np.array_equal(P.list_order(sizes), np.arange(sizes.size))        # the deal order is not the id order
    for nq in P.P_GROUPS_BATCHES:
        fx = P.p_groups(nq)
        assert np.array_equal(fx["vecs"], P.p_groups(16)["vecs"])                # one index serves every batch size
        pl = _plan(fx, fx["nlist"], 0xffffffff)
        assert (pl["list_count"] == nq).all() and (pl["probed"][0][0] == 0)
        assert int(pl["q_nslots"].sum()) <= P.slots_bound(sizes, pl["list_tpc"], fx["nlist"], nq)
        assert len({tuple(q) for q in fx["queries"]}) == nq


@pytest.mark.parametrize("nq", (33, 49))
def test_p_groups_a_swapped_decode_changes_the_answer(nq):
    """chunk = within % ngroups, group = within / ngroups instead of the other way round: rows are scored against the wrong chunks"""
    fx = P.p_groups(nq)
    k = 40
    pl = _plan(fx, fx["nlist"], 0xffffffff)
    truth = _answer(fx, pl, k)
    assert P.same_answer(P.simulate_scan(pl, fx["sizes"], fx["vecs"], fx["queries"], k), truth)
    assert not P.same_answer(P.simulate_scan(pl, fx["sizes"], fx["vecs"], fx["queries"], k, swap_decode=True), truth)
    # the answer draws on more than one chunk of the long list and on more than one list: a dropped item cannot hide
    offs = P.list_offsets(fx["sizes"])
    lists_hit = {int(np.searchsorted(offs, p, side="right")) - 1 for p in truth[0][0]}
    chunks_hit = {int(p - offs[0]) // (4 * P.TILE) for p in truth[0][0] if p < offs[1]}
    assert len(lists_hit) >= 3 and len(chunks_hit) >= 2


def test_exclusion_and_brute_force_restatements():
    fx = P.p_ranks("equal", 40)
    n = fx["vecs"].shape[0]
    ex = P.exclusion(n)
    assert 0.2 < ex.mean() < 0.4
    words = P.pack_bits(ex)
    assert all(bool((int(words[i // 64]) >> (i % 64)) & 1) == bool(ex[i]) for i in range(0, n, 97))
    pl = _plan(fx, 150, 1921)
    pos, _, cnt = _answer(fx, pl, 10, ex)
    assert (cnt == 10).all() and not ex[pos.reshape(-1)].any()
    assert not P.same_answer(_answer(fx, pl, 10, ex), _answer(fx, pl, 10))
    bf = _plan(fx, 200, 0, brute_force=True)
    assert (bf["q_nprobe"] == 200).all() and bf["probed"][7] == list(range(200))

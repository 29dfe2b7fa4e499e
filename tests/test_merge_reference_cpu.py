"""tests/merge_ref.py pinned without a GPU: the model against oracle.merge_topk and against a brute-force sort, the packed layout
against zvec_amd.dist's pack / unpack helpers, and the coverage of merge_kernel's path classes by the shared case tables."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_ref as M  # noqa: E402


@pytest.mark.parametrize("case", M.SHARD_CASES, ids=[c.name for c in M.SHARD_CASES])
def test_model_equals_the_oracle_on_shard_lists(case, oracle):
    table, nparts = M.shard_case(case)
    keys, scores, counts = M.to_strided(table, nparts, case.k)
    wk, ws, wc = M.merge_model_batch(table, case.k)
    ok, os_, oc = oracle.merge_topk(keys, scores, counts, case.k)
    assert oc.tolist() == wc.tolist() == [min(case.k, case.n)] * case.nq
    for q in range(case.nq):                 # (the oracle leaves key 0 behind the count; the model's tail is the kernel's)
        c = int(wc[q])
        assert np.array_equal(ok[q, :c], wk[q, :c]) and np.array_equal(os_[q, :c], ws[q, :c])
        assert np.all(wk[q, c:] == np.uint64(M.KEY_NONE)) and np.all(np.isposinf(ws[q, c:]))
    # the table survives the strided layout
    for a, b in zip(table, M.from_strided(keys, scores, counts)):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def _brute(c, k, threshold, ordinal):
    recs = [(float(c.score[i]), i if ordinal else (int(c.slot[i]), int(c.entry[i])), int(c.key[i]))
            for i in range(c.score.size) if c.valid[i] and c.score[i] <= threshold]
    recs.sort(key=lambda r: r[:2])
    return recs[:k]


@pytest.mark.parametrize("ordinal", [False, True])
def test_model_equals_a_brute_force_sort(ordinal):
    rng = np.random.default_rng(21)
    for _ in range(200):
        n, k = int(rng.integers(0, 40)), int(rng.integers(1, 12))
        c = M.Cands(rng.choice(np.array([-2.0, -0.0, 0.0, 1.0, 1.5], np.float32), n), rng.integers(0, 3, n).astype(np.uint32),
                    rng.integers(0, 4, n).astype(np.uint32), rng.random(n) < 0.8, rng.integers(0, 1 << 40, n).astype(np.uint64))
        thr = float(rng.choice([-2.0, 0.0, 1.0, M.FLT_MAX, np.inf]))
        keys, scores, count = M.merge_model(c, k, thr, ordinal)
        want = _brute(c, k, thr, ordinal)
        assert count == len(want)
        assert scores[:count].tolist() == [r[0] for r in want]
        if ordinal or len({(r[0], r[1]) for r in want}) == len(want):       # (records equal in score, slot and entry may swap keys)
            assert keys[:count].tolist() == [r[2] for r in want]
        assert np.all(keys[count:] == np.uint64(M.KEY_NONE)) and np.all(np.isposinf(scores[count:]))


@pytest.mark.parametrize("pad", [0, 64])
def test_packed_layout_round_trips_through_dist(pad):
    import torch
    from zvec_amd.dist import pack_candidates, unpack_candidates, packed_bytes
    case = next(c for c in M.SHARD_CASES if c.nq == 65 and c.counts == "ragged" and c.n == 129)
    table, nparts = M.shard_case(case)
    keys, scores, counts = M.to_strided(table, nparts, case.k)
    pb = M.packed_bytes(case.nq, case.k)
    assert pb % 16 == 0 and 0 <= pb - packed_bytes(case.nq, case.k) < 16
    buf = M.to_packed(keys, scores, counts, pb + pad)
    # every part's bytes are what pack_candidates writes for that part
    for p in range(nparts):
        mine = pack_candidates(torch.from_numpy(keys[p].astype(np.int64)), torch.from_numpy(scores[p]), torch.from_numpy(counts[p].astype(np.int32)))
        o = p * (pb + pad)
        assert np.array_equal(buf[o:o + mine.numel()], mine.numpy())
        assert np.all(buf[o + mine.numel():o + pb + pad] == 0xa5)
    # and unpack_candidates reads the gathered buffer back (it takes whole strides: the padding rides behind the counts)
    g = torch.from_numpy(buf.reshape(nparts, pb + pad)[:, :packed_bytes(case.nq, case.k)].copy())
    uk, us, uc = unpack_candidates(g, nparts, case.nq, case.k)
    assert np.array_equal(uk.numpy().astype(np.uint64), keys) and np.array_equal(us.numpy(), scores)
    assert np.array_equal(uc.numpy().astype(np.uint32), counts)


def _paths(tables_and_ks):
    return {M.expected_path(c, k, t) for table, k, t in tables_and_ks for c in table}


def test_every_path_class_is_reached_by_every_driver_that_can_reach_it():
    # A: the shard entries take every candidate as a survivor (no pre-bound): all five classes
    a = _paths((M.shard_case(c)[0], c.k, M.FLT_MAX) for c in M.SHARD_CASES)
    assert a == set(M.PATHS)
    # B and C: only the queries whose survivors no pre-bound can cut count (merge_ref.bound_is_moot)
    for make, scores in ((M.flat_list_table, M.chosen_scores()), (M.sparse_list_table, M.sparse_scores())):
        reached = set()
        for case in M.LIST_CASES:
            t = M.list_threshold(case, scores)
            for c in make(M.list_positions(case)):
                if M.bound_is_moot(c, case.k, t):
                    reached.add(M.expected_path(c, case.k, t))
        assert reached == set(M.PATHS)
    # D: the coarse selection over nlist scores and the final merge over nprobe rows; beyond the bound's k <= 64 the row of 129
    # centroids is trimmed or tied, the longer rows overflow, the final merge sorts, and nprobe 129 is general-k
    d = {}
    for case in M.IVF_CASES:
        d.setdefault(case.nprobe > 64, set()).update(M.ivf_paths(case))
    assert d[True] == set(M.PATHS)
    # the exact edges of the two constants
    edge = {c.name: _paths([(M.shard_case(c)[0], c.k, M.FLT_MAX)]) for c in M.SHARD_CASES}
    assert edge["tie128_0-q1-k1-n300"] == {"trim"} and edge["tie129_0-q1-k1-n300"] == {"general-ties"}
    assert edge["tie119_9-q1-k10-n300"] == {"trim"} and edge["tie120_9-q1-k10-n300"] == {"general-ties"}
    assert edge["distinct-q1-k64-n128"] == {"sort"} and edge["distinct-q65-k10-n129"] == {"trim"}
    assert edge["equal-q65-k65-n128"] == {"sort"} and edge["distinct-q1-k1-n513"] == {"general-overflow"}
    assert edge["distinct-q1-k128-n511"] == {"trim"} and edge["distinct-q1-k129-n129"] == {"general-k"}


def test_the_tables_hold_what_the_drivers_need():
    # chosen scores are what the rows give: exact small integers
    rows = M.flat_rows()
    assert rows.shape == (M.STORE_ROWS, 4) and np.array_equal((rows.astype(np.float64) ** 2).sum(1), M.chosen_scores())
    assert np.abs(M.sparse_values()).max() <= 64 and np.all(M.sparse_scores()[M.TIED_ROWS[0]:M.TIED_ROWS[1]] == 64)
    for case in M.LIST_CASES:
        lists = M.list_positions(case)
        assert len(lists) == len(M.VARIANTS) and all(p.size == case.length for p in lists)
    # fewer valid entries than k in a list of 64 or more, a repeated position, holes of every kind
    case = next(c for c in M.LIST_CASES if c.name == "mixed-1024-k10")
    most = M.flat_list_table(M.list_positions(case))[M.VARIANTS.index("most")]
    assert int(most.valid.sum()) == 7 and set(M.HOLES.tolist()) <= set(most.entry.tolist())
    few = M.list_positions(case)[M.VARIANTS.index("few")]
    assert few[0] == few[case.length // 2]
    # every IVF case keeps nprobe below nlist and has ties across the cut
    for case in M.IVF_CASES:
        assert case.nprobe < case.nlist and 1 <= case.nq <= 8
    assert any(np.sort(c.score)[case.nprobe - 1] == np.sort(c.score)[case.nprobe] for case in M.IVF_CASES for c in M.ivf_table(case))

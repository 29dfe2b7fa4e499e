"""The IVF probe plan and the list scan's work items past their first pass, against tests/ivf_plan_ref.py — run with -m gpu.

Every search here is followed by zvec_hip_ctx_last_ivf_plan: the route the host dispatched is asserted, and on the tile route every
array the plan kernels left behind is compared with the plain restatement — exactly, the list-major CSR as sets — before the answer
is compared with the reference top-k and last_stats with the probe rule.  tests/test_ivf_plan_reference_cpu.py holds the fixtures
to what they are there for (probe counts of 64 | 65 | 128 | 129 | 200, two and five scan rounds, every group shape, three chunk
levels) and shows that every forgotten carry changes these answers.

  test                     fixture   what runs past its first pass                                            route
  test_p_ranks_direct      P-ranks   ivf_expand_direct_kernel: 2, 3 and 4 passes of 64 ranks (before_g / _l)  direct, both selections
  test_p_ranks_tile        P-ranks   plan_wave_kernel<false / true>: the same passes (scanned_before,         tile; large-k (k = 500,
                                     slot_carry); ivf_expand_kernel's rank walk; brute force: 4 passes        ivf_expand_kernel)
  test_p_ranks_gaussian    P-ranks   the same on gaussian rows, within the §4 tolerances                      tile
  test_p_rounds            P-rounds  plan_scan_kernel: 2 rounds of 1024 threads, 5 rounds of 256              tile
  test_p_groups            P-groups  the decode: 1 - 4 groups, last group of 1 / 16 / 17 / 32 rows,           tile
                                     1 - 3 chunks on three chunk levels; the host's slots_bound

All rows are small integers (d = 8 or 16): every fp32 score is exact and held bit for bit; a returned key must be a row of a probed
list with exactly the reported score, so among equal scores any row may stand, and nowhere else."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivf_plan_ref as P  # noqa: E402
from tests import util as U  # noqa: E402

pytestmark = pytest.mark.gpu

NO_LIMIT = 0xffffffff
KEY_MUL, KEY_ADD = 7, 1000003              # ivf_plan_ref.keys_for


def _index(fx, dtype="fp32"):
    import zvec_amd as zv
    se = zv.HipIVFSearcher(fx["dim"], "SquaredEuclidean", dtype=dtype)
    n = fx["vecs"].shape[0]
    assert se.load(fx["cent"], P.list_offsets(fx["sizes"]).astype(np.uint64), fx["vecs"], P.keys_for(n)) == 0
    assert se.info() == (n, fx["nlist"])
    return se


def _search_dev(se, ctx, q, k, nprobe, max_scan, excluded=None, stream=None):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, se.np_dtype)).cuda()
    nq = len(q)
    keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    scores = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    counts = torch.zeros(nq, dtype=torch.int32, device="cuda")
    dex = None if excluded is None else torch.from_numpy(P.pack_bits(excluded).view(np.int64)).cuda()
    torch.cuda.synchronize()
    rc = se.search_dev(dq.data_ptr(), nq, k, nprobe, max_scan, keys.data_ptr(), scores.data_ptr(), counts.data_ptr(), ctx,
                       d_exclude=None if dex is None else dex.data_ptr(), stream=stream)
    assert rc == 0
    torch.cuda.synchronize()
    return keys.cpu().numpy().astype(np.uint64), scores.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)


def _reference_plan(fx, got, nprobe, max_scan, brute_force=False):
    """the restatement for this search: the coarse ranking in fp64, the chunk lengths from the read-back's base length"""
    probe, _ = P.coarse_ranking(fx["cent"], fx["queries"], nprobe)
    tpc = got["tpc"] if got.get("tpc") else 2
    ltpc = P.level_tpc(P.list_levels(fx["sizes"]), tpc)
    return P.plan(probe, fx["sizes"], max_scan, ltpc, brute_force=brute_force)


def _check_plan(fx, got, ref, nprobe, what, brute_force=False, scan_threads=1024):
    nq, nlist = len(fx["queries"]), fx["nlist"]
    assert got["route"] == P.ROUTE_TILE, "%s: route %d" % (what, got["route"])
    assert (got["nq"], got["nlist"], got["nprobe"], got["brute_force"]) == (nq, nlist, nlist if brute_force else nprobe, int(brute_force)), what
    assert got["rows_per_group"] == P.ROWS_PER_GROUP and got["scan_threads"] == scan_threads, what
    assert np.array_equal(got["list_tpc"], ref["list_tpc"]), "%s: list_tpc (level_tpc of base length %d)" % (what, got["tpc"])
    for name in ("q_nprobe", "q_scanned", "q_nslots", "slot_begin", "list_count", "list_qoff", "item_off"):
        g, r = got[name].astype(np.int64), ref[name]
        assert g.shape == r.shape, "%s: %s" % (what, name)
        bad = np.nonzero(g != r)[0]
        assert bad.size == 0, "%s: %s differs first at %d: %d vs %d (%d places)" % (what, name, bad[0], g[bad[0]], r[bad[0]], bad.size)
    assert got["total_items"] == ref["total_items"] and got["csr_len"] == int(ref["list_qoff"][nlist]), what
    for l in range(nlist):
        a, b = int(ref["list_qoff"][l]), int(ref["list_qoff"][l + 1])
        pairs = set(zip(got["csr_q"][a:b].tolist(), got["csr_slot"][a:b].tolist()))
        assert pairs == ref["csr"][l], "%s: CSR of list %d" % (what, l)
    # the host's bound dominates what the device dealt, and is what the restated sizing gives
    assert int(ref["slot_begin"][nq]) == int(got["q_nslots"].astype(np.int64).sum()) <= got["slots_bound"], what
    assert got["slots_bound"] == P.slots_bound(fx["sizes"], ref["list_tpc"], nlist if brute_force else nprobe, nq), what


def _check_answer(fx, ref, keys, scores, counts, k, what, excluded=None):
    """counts and scores bit for bit; every key a distinct admitted row of a probed list whose exact score is the reported one"""
    want = P.topk_reference(ref["probed"], fx["sizes"], fx["vecs"], fx["queries"], k, excluded)
    offs = P.list_offsets(fx["sizes"])
    n = fx["vecs"].shape[0]
    assert np.array_equal(counts.astype(np.int64), want[2]), "%s: counts" % what
    for q in range(len(fx["queries"])):
        c = int(want[2][q])
        assert np.array_equal(scores[q, :c].view(np.uint32), want[1][q, :c].astype(np.float32).view(np.uint32)), \
            "%s query %d: scores\n gpu %r\n ref %r" % (what, q, scores[q, :c], want[1][q, :c])
        kq = keys[q, :c].astype(np.int64) - KEY_ADD
        assert (kq % KEY_MUL == 0).all() and (kq >= 0).all() and (kq < n * KEY_MUL).all(), "%s query %d: not keys of this index" % (what, q)
        pos = kq // KEY_MUL
        assert np.unique(pos).size == c, "%s query %d: a row twice" % (what, q)
        lists = np.searchsorted(offs, pos, side="right") - 1
        assert set(lists.tolist()) <= set(ref["probed"][q]), "%s query %d: a row of a list that was not probed" % (what, q)
        assert excluded is None or not excluded[pos].any(), "%s query %d: an excluded row" % (what, q)
        assert np.array_equal(P.scores_of(fx["vecs"][pos], fx["queries"][q]), want[1][q, :c]), "%s query %d: a key with another score" % (what, q)


def _check_stats(se, ctx, ref, what):
    scanned, probes = se.last_stats(ctx, len(ref["q_nprobe"]))
    assert np.array_equal(probes.astype(np.int64), ref["q_nprobe"]), "%s: probes" % what
    assert np.array_equal(scanned.astype(np.int64), ref["q_scanned"]), "%s: scanned" % what


def _run(se, ctx, fx, k, nprobe, max_scan, what, excluded=None, stream=None, scan_threads=1024):
    """one device-pointer search with every check its route allows"""
    nq = len(fx["queries"])
    keys, scores, counts = _search_dev(se, ctx, fx["queries"], k, nprobe, max_scan, excluded, stream)
    got = ctx.last_ivf_plan()
    assert got["route"] == P.expected_route(nq, k, nprobe, fx["sizes"]), "%s: route %d" % (what, got["route"])
    ref = _reference_plan(fx, got, nprobe, max_scan)
    if got["route"] == P.ROUTE_TILE:
        _check_plan(fx, got, ref, nprobe, what, scan_threads=scan_threads)
    else:
        assert "slot_begin" not in got, what                 # nothing to report beyond the route
    if fx["gaussian"]:
        want = P.topk_reference(ref["probed"], fx["sizes"], fx["vecs"], fx["queries"], k, excluded)
        wk = P.keys_for(fx["vecs"].shape[0])[np.maximum(want[0], 0)]
        qn = (fx["queries"].astype(np.float64) ** 2).sum(1)
        bn = (fx["vecs"].astype(np.float64) ** 2).sum(1).max()
        U.tie_tolerant_compare(keys, scores, counts, wk, want[1].astype(np.float32), want[2], rtol=2e-6, atol=1e-6,
                               select_band=4e-6 * (qn + bn), what=what)
    else:
        _check_answer(fx, ref, keys, scores, counts, k, what, excluded)
    if got["route"] != P.ROUTE_LARGE_K:                      # (the large-k route keeps no per-query statistics)
        _check_stats(se, ctx, ref, what)
    return got, ref


# ---- P-ranks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", ("equal", "unequal"))
def test_p_ranks_direct(sizes):
    """4 queries: ivf_expand_direct_kernel walks 150 (200) ranks in passes of 64 and must stop at rank 64, 65, 128, 129 (200) for 30-row
    lists, at a rank of its own for every query of the 1 ... 59-row lists; k = 10 leaves the selection to the scoring blocks, k = 100
    to the two-step selection over the score matrix"""
    fx = P.p_ranks(sizes, 4)
    se = _index(fx)
    ctx = se.create_context()
    for nprobe, max_scan in P.P_RANKS_PAIRS:
        what = "direct %s nprobe %d max_scan %d" % (sizes, nprobe, max_scan)
        got, ref = _run(se, ctx, fx, 10, nprobe, max_scan, what)
        assert got["route"] == P.ROUTE_DIRECT_BLOCK_TOPK
        if sizes == "equal":
            assert (ref["q_nprobe"] == P.P_RANKS_PROBED[(nprobe, max_scan)]).all()
    got, _ = _run(se, ctx, fx, 100, 150, 3841, "direct %s k 100" % sizes)
    assert got["route"] == P.ROUTE_DIRECT_SELECT
    _run(se, ctx, fx, 10, 150, 1921, "direct %s excluded" % sizes, excluded=P.exclusion(fx["vecs"].shape[0]))
    _run(se, ctx, fx, 500, 150, 3841, "direct %s k 500" % sizes)


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
@pytest.mark.parametrize("sizes", ("equal", "unequal"))
def test_p_ranks_tile(sizes, dtype):
    """40 queries: plan_wave_kernel counts and fills in passes of 64 ranks; the read-back shows every array it and plan_scan_kernel
    wrote.  fp32 adds k = 500 (ivf_expand_kernel's serial rank walk, with and without exclusion), an exclusion bitset and search_bf
    (every list in id order: four passes, no probe rule) for 40 and for 4 queries."""
    fx = P.p_ranks(sizes, 40)
    se = _index(fx, dtype)
    ctx = se.create_context()
    n = fx["vecs"].shape[0]
    for nprobe, max_scan in P.P_RANKS_PAIRS:
        what = "tile %s %s nprobe %d max_scan %d" % (dtype, sizes, nprobe, max_scan)
        got, ref = _run(se, ctx, fx, 10, nprobe, max_scan, what)
        assert got["route"] == P.ROUTE_TILE
        if sizes == "equal":
            assert (got["q_nprobe"] == P.P_RANKS_PROBED[(nprobe, max_scan)]).all()
    _run(se, ctx, fx, 10, 150, 1921, "tile %s %s excluded" % (dtype, sizes), excluded=P.exclusion(n))
    if dtype == "fp16":
        return
    for ex in (None, P.exclusion(n)):
        got, _ = _run(se, ctx, fx, 500, 150, 3841, "large k %s%s" % (sizes, "" if ex is None else " excluded"), excluded=ex)
        assert got["route"] == P.ROUTE_LARGE_K
    for nq in (40, 4):
        sub = dict(fx, queries=fx["queries"][:nq])
        ctx.set_topk(10)
        assert se.search_bf_impl(sub["queries"], nq, ctx) == 0
        got = ctx.last_ivf_plan()
        what = "search_bf %s %d queries" % (sizes, nq)
        ltpc = P.level_tpc(P.list_levels(fx["sizes"]), got["tpc"])
        ref = P.plan([None] * nq, fx["sizes"], 0, ltpc, brute_force=True)
        _check_plan(sub, got, ref, 1, what, brute_force=True)
        assert (got["q_nprobe"] == fx["nlist"]).all() and (got["q_scanned"] == n).all()
        _check_answer(sub, ref, ctx.keys, ctx.scores, ctx.counts, 10, what)
        _check_stats(se, ctx, ref, what)


def test_p_ranks_gaussian():
    """the equal-size fixture on gaussian rows (the line coordinate of centroids and queries kept: the coarse ranking stays exact):
    the plan is compared exactly, the answer within the tolerances of test_ivf_gpu_build_then_same_index_on_oracle"""
    fx = P.p_ranks("equal", 40, gaussian=True)
    se = _index(fx)
    ctx = se.create_context()
    for nprobe, max_scan in ((150, 1921), (150, 3841)):
        got, _ = _run(se, ctx, fx, 10, nprobe, max_scan, "gaussian nprobe %d max_scan %d" % (nprobe, max_scan))
        assert got["route"] == P.ROUTE_TILE


# ---- P-rounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ("own", "caller"))
def test_p_rounds(stream):
    """1061 queries over 1064 lists: slot_begin, list_qoff and item_off are scanned in two rounds of 1024 threads on the context's own
    stream and in five rounds of 256 on a caller's; the list scan's item search runs over 1064 entries with runs of zero-item lists
    across 255 | 256, 1023 | 1024 and at both ends"""
    import torch
    fx = P.p_rounds()
    se = _index(fx)
    ctx = se.create_context()
    threads = 1024 if stream == "own" else 256
    s = None if stream == "own" else torch.cuda.Stream()
    got, ref = _run(se, ctx, fx, 5, P.P_ROUNDS_NPROBE, NO_LIMIT, "rounds %s" % stream, stream=None if s is None else s.cuda_stream,
                    scan_threads=threads)
    assert got["scan_threads"] == threads and got["nq"] > threads and got["nlist"] > threads
    items = np.diff(got["item_off"].astype(np.int64))
    assert (items[list(P.P_ROUNDS_UNPROBED)] == 0).all() and (items[list(P.P_ROUNDS_EMPTY)] == 0).all() and got["total_items"] > 1024


# ---- P-groups ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
def test_p_groups(dtype):
    """every list probed by the whole batch: 1 to 4 groups of 32 query rows with a last group of 1, 16, 17 or 32 rows (both sides of
    the scan's half switch), lists of 1, 127, 128, 129, 500 and 1153 rows on three chunk levels — 1, 2 and 3 chunks"""
    se = ctx = None
    levels = P.list_levels(P.P_GROUPS_SIZES)
    big = int(np.argmax(P.P_GROUPS_SIZES))
    for nq in P.P_GROUPS_BATCHES:
        fx = P.p_groups(nq)
        if se is None:                                    # (the rows do not depend on the batch: one index)
            se = _index(fx, dtype)
            ctx = se.create_context()
        what = "groups %s %d queries" % (dtype, nq)
        got, ref = _run(se, ctx, fx, 40, fx["nlist"], NO_LIMIT, what)
        assert (got["list_count"] == nq).all(), what
        for lv in (0, 1, 2):                              # all three levels occur, each with the chunk length level_tpc gives it
            assert (got["list_tpc"][levels == lv] == P.level_tpc([lv], got["tpc"])[0]).all() and (levels == lv).any(), what
        assert len(set(got["list_tpc"].tolist())) == 3, what
        assert ref["chunks"][big] > 1 and got["q_nslots"][0] == ref["chunks"].sum(), what
        groups, _ = P.group_shapes(nq)
        assert got["total_items"] == groups * int(ref["chunks"].sum()), what
        # the host's bound in the form it is computed: the nprobe lists with the most chunks, times the batch
        assert int(got["q_nslots"].astype(np.int64).sum()) <= got["slots_bound"] == int(ref["chunks"].sum()) * nq, what


def test_read_back_has_nothing_to_report_after_another_search():
    """the plan belongs to the LAST search of the context: a flat search in between leaves nothing to report, and so does a context
    that has not searched"""
    import zvec_amd as zv
    fx = P.p_groups(16)
    se = _index(fx)
    ctx = se.create_context()
    assert ctx.last_ivf_plan()["route"] == P.ROUTE_NONE
    _run(se, ctx, fx, 10, fx["nlist"], NO_LIMIT, "before the flat search")
    flat = zv.HipFlatSearcher(fx["dim"], "SquaredEuclidean")
    assert flat.load(fx["vecs"][:200]) == 0
    ctx.set_topk(3)
    assert flat.search_impl(fx["queries"], 16, ctx) == 0
    got = ctx.last_ivf_plan()
    assert got["route"] == P.ROUTE_NONE and "slot_begin" not in got

"""merge_kernel (zvec_amd/csrc/zvk_merge.hip.h) on every candidate-stream layout, pre-bound, survivor path, launch width and tie
rule, against the model of its contract in tests/merge_ref.py — run with -m gpu.

Four drivers reach the kernel: A the shard-merge entries (strided and packed lists with counts, 64 threads), B the flat by-positions
search (one contiguous slot, the dense-row bound), C the sparse by-ids search (every candidate a slot, the bound over slot heads, 256
and 64 threads), D the IVF small-batch route (dense-row selection at 256 threads, then a merge in stream order).

All data is small integers (|v| <= 64, dim <= 4; the shard entries take their scores as given), so every score is exact in fp32
under any summation order, and every assertion is exact equality of keys, counts and score values, the padded tail included.  Inputs
never hold NaN, nor +inf as a real score.
"""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -12, -31
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zv():
    import zvec_amd
    return zvec_amd


@pytest.fixture(scope="module")
def ctx(zv):
    from zvec_amd.index import IndexContext
    return IndexContext(0)


# ---- A. the shard-merge entries ---------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _dev_out(nq, k):
    import torch
    return (torch.full((nq, k), 0x1234, dtype=torch.int64, device="cuda"), torch.full((nq, k), -77.0, dtype=torch.float32, device="cuda"),
            torch.full((nq,), 99, dtype=torch.int32, device="cuda"))


def _host_out(out):
    return out[0].cpu().numpy().view(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _merge_host(ctx, keys, scores, counts, k):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    nparts, nq = counts.shape
    ok, os_, oc = np.full((nq, k), 0x1234, np.uint64), np.full((nq, k), -77.0, np.float32), np.full(nq, 99, np.uint32)
    rc = _lib.lib().zvec_hip_merge_topk(ctx._h, _np_ptr(keys), _np_ptr(scores), _np_ptr(counts), nparts, nq, k, _np_ptr(ok), _np_ptr(os_), _np_ptr(oc))
    return rc, (ok, os_, oc)


def _merge_dev(ctx, keys, scores, counts, k):
    import torch
    from zvec_amd import _lib
    nparts, nq = counts.shape
    dk, ds, dc = _dev(keys), _dev(scores), _dev(counts)
    out = _dev_out(nq, k)
    torch.cuda.synchronize()
    rc = _lib.lib().zvec_hip_merge_topk_dev(ctx._h, _p(dk), _p(ds), _p(dc), nparts, nq, k, _p(out[0]), _p(out[1]), _p(out[2]), None)
    ctx.synchronize()
    return rc, _host_out(out)


def _merge_packed(ctx, keys, scores, counts, k, pad=0, stride=None, nparts=None, topk=None):
    import torch
    from zvec_amd import _lib
    nq = counts.shape[1]
    pb = int(_lib.lib().zvec_hip_packed_bytes(nq, k))
    assert pb == M.packed_bytes(nq, k)
    buf = _dev(M.to_packed(keys, scores, counts, pb + pad))
    out = _dev_out(nq, k)
    torch.cuda.synchronize()
    rc = _lib.lib().zvec_hip_merge_topk_packed_dev(ctx._h, _p(buf), pb + pad if stride is None else stride, counts.shape[0] if nparts is None else nparts,
                                                   nq, k if topk is None else topk, _p(out[0]), _p(out[1]), _p(out[2]), None)
    ctx.synchronize()
    return rc, _host_out(out)


@pytest.mark.parametrize("case", M.SHARD_CASES, ids=[c.name for c in M.SHARD_CASES])
def test_shard_entries_equal_the_model_and_each_other(case, ctx):
    table, nparts = M.shard_case(case)
    keys, scores, counts = M.to_strided(table, nparts, case.k)
    want = M.merge_model_batch(table, case.k)
    results = [("host", _merge_host(ctx, keys, scores, counts, case.k)), ("dev", _merge_dev(ctx, keys, scores, counts, case.k)),
               ("packed", _merge_packed(ctx, keys, scores, counts, case.k)), ("packed + 64", _merge_packed(ctx, keys, scores, counts, case.k, pad=64))]
    for what, (rc, got) in results:
        assert rc == 0, what
        M.assert_same(got, want, "%s %s" % (case.name, what))
    for what, (rc, got) in results[1:]:
        M.assert_same(got, results[0][1][1], "%s %s against host" % (case.name, what))


def test_packed_entry_refusals(ctx):
    case = next(c for c in M.SHARD_CASES if c.name == "distinct-q65-k10-n129")
    table, nparts = M.shard_case(case)
    keys, scores, counts = M.to_strided(table, nparts, case.k)
    pb = M.packed_bytes(case.nq, case.k)
    for kw in (dict(stride=pb - 8), dict(stride=pb - 16), dict(pad=64, stride=pb + 4), dict(nparts=0), dict(topk=0)):
        rc, (gk, gs, gc) = _merge_packed(ctx, keys, scores, counts, case.k, **kw)
        assert rc == INVALID, kw
        assert np.all(gk == 0x1234) and np.all(gs == -77.0) and np.all(gc == 99)          # no output is touched


# ---- k ceiling --------------------------------------------------------------------------------
def _lds_caps():
    """(search paths, shard-merge entries): the two caps of merge_lds_bytes(k) = 12 k + 16, from the header that sets them"""
    src = open(os.path.join(ROOT, "zvec_amd", "csrc", "api_flat_scan.inc.h")).read()
    m = re.search(r"MERGE_LDS_MAX = (\d+) \* 1024, SHARD_MERGE_LDS_MAX = (\d+) \* 1024", src)
    assert m and "return (size_t)k * 12 + 16" in src
    return int(m.group(1)) * 1024, int(m.group(2)) * 1024


def _ceiling_case(k):
    """two parts, two queries: lists longer than any survivor path takes, with ties across the parts"""
    rng = np.random.default_rng(k)
    table = []
    for q in range(2):
        cnt = np.array([k - 7 * q, k // 2 + q])
        slot = np.repeat(np.arange(2, dtype=np.uint32), cnt)
        entry = np.concatenate([np.arange(c, dtype=np.uint32) for c in cnt])
        n = int(cnt.sum())
        table.append(M.Cands(rng.integers(-500, 500, n).astype(np.float32), slot, entry, np.ones(n, bool),
                             rng.permutation(n).astype(np.uint64) + np.uint64(1 << 35)))
    return table


def test_largest_k_of_the_shard_entries(ctx):
    kmax = (_lds_caps()[1] - 16) // 12
    table = _ceiling_case(kmax)
    keys, scores, counts = M.to_strided(table, 2, kmax)
    want = M.merge_model_batch(table, kmax)
    assert want[2].tolist() == [kmax, kmax]
    for what, fn in (("host", _merge_host), ("dev", _merge_dev), ("packed", _merge_packed)):
        rc, got = fn(ctx, keys, scores, counts, kmax)
        assert rc == 0, "%s: k = %d does not launch (rc %d)" % (what, kmax, rc)
        M.assert_same(got, want, "k = %d %s" % (kmax, what))
    keys, scores, counts = M.to_strided(_ceiling_case(kmax + 1), 2, kmax + 1)
    for fn in (_merge_host, _merge_dev, _merge_packed):
        assert fn(ctx, keys, scores, counts, kmax + 1)[0] == UNSUPPORTED


# ---- B. flat by-positions ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat_store():
    import zvec_amd as zv
    st = zv.HipFlatStreamer(4, "SquaredEuclidean")
    assert st.add_batch(M.flat_rows(), M.store_keys()) == 0 and st.count() == M.STORE_ROWS
    return st


def _flat_search(lists, k, threshold):
    st = _flat_store()
    c = st.create_context()
    c.set_topk(k)
    c.set_threshold(threshold)
    rc = st.search_by_positions_impl(np.zeros((len(lists), 4), np.float32), lists, len(lists), c)
    return rc, (c.keys, c.scores, c.counts)


@pytest.mark.parametrize("case", M.LIST_CASES, ids=[c.name for c in M.LIST_CASES])
def test_flat_by_positions(case):
    lists = M.list_positions(case)
    thr = M.list_threshold(case, M.chosen_scores())
    want = M.merge_model_batch(M.flat_list_table(lists), case.k, thr)
    if case.threshold == "below":
        assert not want[2].any()
    rc, got = _flat_search(lists, case.k, thr)
    assert rc == 0
    M.assert_same(got, want, case.name)
    # lists of unequal length in one call: the shorter ones end in an unused tail
    mixed = [lists[0], lists[1][:max(1, case.length // 3)], lists[2][:max(1, case.length - 1)]]
    rc, got = _flat_search(mixed, case.k, thr)
    assert rc == 0
    M.assert_same(got, M.merge_model_batch(M.flat_list_table(mixed), case.k, thr), case.name + " unequal")


def test_flat_ties_are_broken_by_position_and_a_repeat_is_returned_twice():
    a, b = M.TIED_ROWS
    lists = [np.array([b - 1, a + 5, a + 5, a, 1001, 1000, 3, M.STORE_ROWS, a + 2], np.uint32)]
    rc, (keys, scores, counts) = _flat_search(lists, 8, M.FLT_MAX)
    assert rc == 0 and counts.tolist() == [8]
    assert keys[0].tolist() == M.store_keys()[[3, 1000, 1001, a, a + 2, a + 5, a + 5, b - 1]].tolist()
    assert scores[0].tolist() == [1.0] + [500.0] * 7


def test_largest_k_of_the_search_paths():
    kmax = (_lds_caps()[0] - 16) // 12
    lists = [np.array([5, 4, M.STORE_ROWS, 1030, 1025, 9, 9, 2000], np.uint32), np.arange(300, 0, -1).astype(np.uint32)]
    rc, got = _flat_search(lists, kmax, M.FLT_MAX)
    assert rc == 0, "k = %d does not launch (rc %d)" % (kmax, rc)
    M.assert_same(got, M.merge_model_batch(M.flat_list_table(lists), kmax), "k = %d" % kmax)
    assert _flat_search(lists, kmax + 1, M.FLT_MAX)[0] == UNSUPPORTED


# ---- C. sparse by-ids -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sparse_store():
    import zvec_amd as zv
    se = zv.HipFlatSparseStreamer()
    n = M.STORE_ROWS
    assert se.add_batch(np.ones(n, np.uint32), (np.arange(n) % 2).astype(np.uint32), M.sparse_values().astype(np.float32), M.store_keys()) == 0
    assert se.count() == n
    return se


def _sparse_search(lists, k, threshold):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    se = _sparse_store()
    nq = len(lists)
    qc, qi, qv = np.full(nq, 2, np.uint32), np.tile(np.array([0, 1], np.uint32), nq), np.tile(np.array([1.0, 64.0], np.float32), nq)
    ids = np.ascontiguousarray(np.concatenate(lists), np.uint32)
    offsets = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint32)
    keys, scores, counts = np.full((nq, k), 0x1234, np.uint64), np.full((nq, k), -77.0, np.float32), np.full(nq, 99, np.uint32)
    rc = _lib.lib().zvec_hip_sparse_search_by_ids(se._h, None, _np_ptr(qc), _np_ptr(qi), _np_ptr(qv), nq, _np_ptr(ids), _np_ptr(offsets), k,
                                                  float(threshold), None, _np_ptr(keys), _np_ptr(scores), _np_ptr(counts))
    return rc, (keys, scores, counts)


@pytest.mark.parametrize("case", M.LIST_CASES, ids=[c.name for c in M.LIST_CASES])
def test_sparse_by_ids_at_both_launch_widths(case):
    lists = M.list_positions(case)
    assert len(lists) == 3
    thr = M.list_threshold(case, M.sparse_scores())
    want = M.merge_model_batch(M.sparse_list_table(lists), case.k, thr)
    if case.threshold == "below":
        assert not want[2].any()
    rc, got = _sparse_search(lists, case.k, thr)                  # 3 queries: 256 threads, the waves append through one counter
    assert rc == 0
    M.assert_same(got, want, case.name + " x3")
    many = [lists[q % 3] for q in range(257)]                     # 257 queries: 64 threads
    rc, got257 = _sparse_search(many, case.k, thr)
    assert rc == 0
    M.assert_same(got257, tuple(np.stack([w[q % 3] for q in range(257)]) for w in want), case.name + " x257")
    M.assert_same(tuple(g[:3] for g in got257), got, case.name + " x257 against x3")


def test_sparse_ties_are_broken_by_list_order():
    a, b = M.TIED_ROWS
    best = int(np.argmin(M.sparse_scores()))
    lists = [np.array([b - 1, a + 5, a + 5, a, M.STORE_ROWS, a + 2, best], np.uint32)] * 3
    rc, (keys, scores, counts) = _sparse_search(lists, 6, M.FLT_MAX)
    assert rc == 0 and counts.tolist() == [6] * 3
    assert keys[0].tolist() == M.store_keys()[[best, b - 1, a + 5, a + 5, a, a + 2]].tolist()
    assert scores[0, 1:].tolist() == [64.0] * 5


def test_sparse_by_ids_beyond_the_fused_lists():
    """topk above SPARSE_FUSED_MAX_K = 128 through the same entry"""
    lists = M.list_positions(next(c for c in M.LIST_CASES if c.name == "mixed-1025-k129"))
    rc, got = _sparse_search(lists, 300, M.FLT_MAX)
    assert rc == 0
    M.assert_same(got, M.merge_model_batch(M.sparse_list_table(lists), 300), "k 300")


# ---- D. the IVF small-batch route as a dense-row selector --------------------------------------
@functools.lru_cache(maxsize=None)
def _ivf(nlist):
    import zvec_amd as zv
    ivf = zv.HipIVFSearcher(1, "SquaredEuclidean", device=0)
    cent = M.ivf_centroids(nlist)
    assert ivf.load(cent, np.arange(nlist + 1, dtype=np.uint64), cent, M.ivf_keys(nlist)) == 0
    return ivf


@pytest.mark.parametrize("case", M.IVF_CASES, ids=[c.name for c in M.IVF_CASES])
def test_ivf_small_batch_route_is_the_coarse_selection(case):
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    ivf = _ivf(case.nlist)
    c = ivf.create_context()
    q = M.ivf_queries(case)
    k = case.nprobe
    want = M.merge_model_batch(M.ivf_table(case), k)
    assert want[2].tolist() == [k] * case.nq
    for thr in (M.FLT_MAX, float("inf")):
        keys, scores, counts = np.full((case.nq, k), 0x1234, np.uint64), np.full((case.nq, k), -77.0, np.float32), np.full(case.nq, 99, np.uint32)
        rc = _lib.lib().zvec_hip_ivf_search(ivf._h, c._h, _np_ptr(q), case.nq, k, thr, case.nprobe, 0xffffffff, None, _np_ptr(keys),
                                            _np_ptr(scores), _np_ptr(counts))
        assert rc == 0
        probes = ivf.last_stats(c, case.nq)[1]
        assert probes.tolist() == [case.nprobe] * case.nq       # (no other route)
        M.assert_same((keys, scores, counts), want, "%s threshold %r" % (case.name, thr))


def test_ivf_small_batch_ties_follow_the_probe_order_not_the_positions(zv):
    """every probed row scores the same, and the probe order (centroids by distance, lower id first) is not the order of the rows'
    positions: the final merge orders equal scores by their place in the candidate stream"""
    from zvec_amd import _lib
    from zvec_amd.index import _np_ptr
    nlist, nprobe = 65, 10
    cent = np.arange(nlist, dtype=np.float32).reshape(nlist, 1)
    rows = np.where(np.arange(nlist) < 32, 57.0, 7.0).astype(np.float32).reshape(nlist, 1)          # (32 - 57)^2 == (32 - 7)^2
    ivf = zv.HipIVFSearcher(1, "SquaredEuclidean", device=0)
    assert ivf.load(cent, np.arange(nlist + 1, dtype=np.uint64), rows, M.ivf_keys(nlist)) == 0
    c = ivf.create_context()
    q = np.full((1, 1), 32.0, np.float32)
    keys, scores, counts = np.zeros((1, nprobe), np.uint64), np.zeros((1, nprobe), np.float32), np.zeros(1, np.uint32)
    rc = _lib.lib().zvec_hip_ivf_search(ivf._h, c._h, _np_ptr(q), 1, nprobe, M.FLT_MAX, nprobe, 0xffffffff, None, _np_ptr(keys), _np_ptr(scores),
                                        _np_ptr(counts))
    assert rc == 0 and counts.tolist() == [nprobe] and ivf.last_stats(c, 1)[1].tolist() == [nprobe]
    assert keys[0].tolist() == M.ivf_keys(nlist)[[32, 31, 33, 30, 34, 29, 35, 28, 36, 27]].tolist()
    assert scores[0].tolist() == [625.0] * nprobe

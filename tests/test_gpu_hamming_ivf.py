"""Binary rows under the Hamming metric through inverted lists on the GPU (zvec_hip_bivf_*), against tests/hamming_ivf_ref.py.
Everything is exact: probe orders, probe counts and scanned rows with np.array_equal; result lists with check_hamming_lists and
the model's admissible matrix (only the membership and order of EQUAL scores is left free)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ivf_ref as R  # noqa: E402
from hamming_ref import check_hamming_lists, hamming_reference  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED, MISMATCH, INVALID, NO_INDEX_LOADED, NO_READY = -12, -24, -31, -204, -21
NO_CUT = 0xffffffff


def _searcher(dim, dtype="binary32"):
    import zvec_amd as zv
    return zv.HipHammingIVFSearcher(dim, dtype=dtype)


def _loaded(cent, offs, rows, dim, keys=None, dtype="binary32"):
    se = _searcher(dim, dtype)
    assert se.load(cent, offs, rows, keys) == 0
    assert se.info() == (rows.shape[0], cent.shape[0])
    return se


def _search(se, q, k, nprobe, max_scan=NO_CUT, threshold=None, exclude=None, ctx=None):
    ctx = ctx or se.create_context()
    ctx.set_topk(k)
    if threshold is not None:
        ctx.set_threshold(threshold)
    if exclude is not None:
        ctx.set_exclude_bitset(R.words_of(exclude))
    assert se.search_impl(q, q.shape[0], ctx, nprobe=nprobe, max_scan=max_scan) == 0
    return ctx.keys, ctx.scores, ctx.counts, se.last_probes(ctx, q.shape[0], nprobe)


def _check(se, cent, offs, rows, q, k, nprobe, max_scan=NO_CUT, threshold=None, exclude=None, keys=None, what=""):
    """one search against the model: probe order, probe count, scanned rows, result lists"""
    got_k, got_s, got_c, (pidx, pcnt, pscan) = _search(se, q, k, nprobe, max_scan, threshold, exclude)
    order, cnt, scanned, adm = R.model(cent, offs, q, nprobe, max_scan, exclude)
    assert np.array_equal(pidx, order), what
    assert np.array_equal(pcnt, cnt), what
    assert np.array_equal(pscan, scanned), what
    ref = hamming_reference(rows, q) if rows.shape[0] else np.zeros((q.shape[0], 0), np.int64)
    check_hamming_lists(got_k, got_s, got_c, ref, k, threshold=threshold, admissible=adm, key_of_row=keys, what=what)
    return got_k, got_s, got_c, adm, ref


@pytest.mark.parametrize("dim", [32, 96, 160, 224, 864])
def test_every_chunk_path_on_ragged_lists(dim):
    """list lengths 0, 1, 127, 128, 129, 300 in one index: lists start and end off the tile grid, one spans three tiles"""
    rng = np.random.default_rng(dim)
    cent, offs, rows = R.index_of(rng, dim, R.RAGGED)
    se = _loaded(cent, offs, rows, dim)
    q = np.concatenate([R.bits(rng, 5, dim), cent[[1, 2, 5]], rows[[0, 127, 128, 684]]])
    for nprobe in (1, 3, 6, 9):                         # (9: clamped to nlist)
        _check(se, cent, offs, rows, q, 10, nprobe, what="dim=%d nprobe=%d" % (dim, nprobe))
    assert np.array_equal(se.get_vectors_by_ids(np.arange(685)), rows)


def test_binary64():
    rng = np.random.default_rng(64)
    cent, offs, rows = R.index_of(rng, 128, R.RAGGED, dtype="binary64")
    assert rows.dtype == np.uint64 and rows.shape[1] == 2
    se = _loaded(cent, offs, rows, 128, dtype="binary64")
    q = np.concatenate([R.bits(rng, 6, 128, "binary64"), cent[[3]]])
    _check(se, cent, offs, rows, q, 10, 3)
    assert np.array_equal(se.get_vectors_by_ids([0, 300, 684]), rows[[0, 300, 684]])


@pytest.mark.parametrize("nlist", [1, 5, 70])
def test_list_counts(nlist):
    """one list; a few; more lists than lanes"""
    rng = np.random.default_rng(nlist)
    lengths = rng.integers(0, 40, nlist)
    lengths[0] = 33
    cent, offs, rows = R.index_of(rng, 96, tuple(int(x) for x in lengths))
    se = _loaded(cent, offs, rows, 96)
    q = np.concatenate([R.bits(rng, 9, 96), cent[:3]])
    for nprobe in (1, nlist, nlist + 3):
        _check(se, cent, offs, rows, q, 10, nprobe, what="nlist=%d nprobe=%d" % (nlist, nprobe))


@pytest.mark.parametrize("nq", [1, 33, 70])
def test_more_than_a_query_block_on_one_list(nq):
    cent, offs, rows, q = R.crowded_lists(np.random.default_rng(3), nq)
    se = _loaded(cent, offs, rows, 96)
    _check(se, cent, offs, rows, q, 10, 2, what="nq=%d" % nq)
    _check(se, cent, offs, rows, q, 10, 1, what="nq=%d nprobe=1" % nq)


def test_duplicate_centroids_probe_the_lower_index():
    cent, offs, rows, q = R.duplicate_centroids(np.random.default_rng(2))
    se = _loaded(cent, offs, rows, 96)
    _, _, _, (pidx, pcnt, _) = _search(se, q, 5, 1)
    assert np.all(pidx[:, 0] == 1) and np.all(pcnt == 1)
    _check(se, cent, offs, rows, q, 5, 1)
    _check(se, cent, offs, rows, q, 5, 2)


def test_max_scan_count():
    cent, offs, rows, q, nprobe, length = R.max_scan_case(np.random.default_rng(4))
    se = _loaded(cent, offs, rows, 96)
    for max_scan in (length, length + 1, 0, 1, NO_CUT):
        _, _, got_c, _, _ = _check(se, cent, offs, rows, q, 10, nprobe, max_scan=max_scan, what="max_scan=%d" % max_scan)
        if max_scan == 0:
            assert not got_c.any()


@pytest.mark.parametrize("k", [1, 10, 128])
def test_k(k):
    rng = np.random.default_rng(k)
    cent, offs, rows = R.index_of(rng, 96, R.RAGGED)
    se = _loaded(cent, offs, rows, 96)
    q = np.concatenate([R.bits(rng, 4, 96), cent[[1, 5]]])
    _check(se, cent, offs, rows, q, k, 6)
    # topk larger than the probed rows: short counts
    _, _, got_c, adm, _ = _check(se, cent, offs, rows, q, k, 1)
    if k == 128:
        assert np.array_equal(got_c, np.minimum(adm.sum(axis=1), k)) and np.any(got_c < k)


def test_k_129_is_unsupported():
    from zvec_amd import _lib
    cent, offs, rows = R.index_of(np.random.default_rng(9), 96, R.RAGGED)
    se = _loaded(cent, offs, rows, 96)
    ctx = se.create_context()
    ctx.set_topk(129)
    assert se.search_impl(rows[:2], 2, ctx, nprobe=2, max_scan=NO_CUT) == UNSUPPORTED
    dummy = np.zeros(4096, np.uint64)
    assert _lib.lib().zvec_hip_bivf_search_dev(se._h, ctx._h, dummy.ctypes.data, 1, 129, C.c_float(1e9), 1, NO_CUT, None, dummy.ctypes.data,
                                               dummy.ctypes.data, dummy.ctypes.data, None) == UNSUPPORTED


def test_threshold():
    rng = np.random.default_rng(14)
    cent, offs, rows = R.index_of(rng, 96, R.RAGGED)
    se = _loaded(cent, offs, rows, 96)
    q = np.concatenate([R.bits(rng, 3, 96), cent[[5]]])
    _, _, _, adm, ref = _check(se, cent, offs, rows, q, 100, 3)
    r = int(np.sort(ref[3][adm[3]])[60])                # an occurring distance of a probed row
    assert r > 0
    for radius in (float(r), float(r - 1), float(r) - 0.5, float(r + 1), -1.0):
        _check(se, cent, offs, rows, q, 100, 3, threshold=radius, what="radius=%r" % radius)
    _, s, c, _ = _search(se, q, 100, 3, threshold=float(r))
    assert s[3, c[3] - 1] == r                          # the radius itself is kept


def test_exclude_bits():
    rng = np.random.default_rng(15)
    cent, offs, rows = R.index_of(rng, 96, R.RAGGED)
    se = _loaded(cent, offs, rows, 96)
    q = np.concatenate([R.bits(rng, 4, 96), cent[[4, 5]]])
    whole_list = np.zeros(685, bool)
    whole_list[int(offs[5]):int(offs[6])] = True        # all of the longest list
    alternating = np.arange(685) % 2 == 0
    for ex in (whole_list, alternating, np.ones(685, bool)):
        _, _, got_c, adm, _ = _check(se, cent, offs, rows, q, 12, 3, exclude=ex)
        assert not adm[:, ex].any()
    assert not got_c.any()


def test_caller_keys_and_search_dev():
    import torch
    rng = np.random.default_rng(19)
    cent, offs, rows = R.index_of(rng, 160, R.RAGGED)
    keys = (rng.permutation(685) + 10_000).astype(np.uint64)
    se = _loaded(cent, offs, rows, 160, keys=keys)
    q = np.concatenate([R.bits(rng, 38, 160), cent[[2, 5]]])
    k, nprobe = 10, 3
    hk, hs, hc, adm, ref = _check(se, cent, offs, rows, q, k, nprobe, keys=keys)
    assert hk[hc > 0].min() >= 10_000
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q.view(np.int32)).to(dev)
    dk = torch.zeros((40, k), dtype=torch.int64, device=dev)
    ds = torch.zeros((40, k), dtype=torch.float32, device=dev)
    dc = torch.zeros((40,), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    ctx = se.create_context()
    assert se.search_dev(dq.data_ptr(), 40, k, nprobe, NO_CUT, dk.data_ptr(), ds.data_ptr(), dc.data_ptr(), ctx, stream=stream.cuda_stream) == 0
    stream.synchronize()
    gk, gs, gc = dk.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dc.cpu().numpy().view(np.uint32)
    check_hamming_lists(gk, gs, gc, ref, k, admissible=adm, key_of_row=keys)
    assert np.array_equal(gs, hs) and np.array_equal(gc, hc)


def test_two_slices_equal_one():
    from zvec_amd import _lib
    cent, offs, rows, q, nprobe, k, cap = R.two_slices(np.random.default_rng(6))
    se = _loaded(cent, offs, rows, 96)
    _, one_s, one_c, adm, ref = _check(se, cent, offs, rows, q, k, nprobe)
    L = _lib.lib()
    assert L.zvec_hip_set_option(b"bivf_part_bytes", cap) == 0
    try:
        _, two_s, two_c, _, _ = _check(se, cent, offs, rows, q, k, nprobe, what="two slices")
    finally:
        assert L.zvec_hip_set_option(b"bivf_part_bytes", 1 << 30) == 0
    assert np.array_equal(one_s, two_s) and np.array_equal(one_c, two_c)


@pytest.fixture(scope="module")
def built():
    rng = np.random.default_rng(30)
    proto = R.bits(rng, 12, 96)
    rows = np.repeat(proto, 50, axis=0) ^ (R.bits(rng, 600, 96) & R.bits(rng, 600, 96) & R.bits(rng, 600, 96))
    rows = rows[rng.permutation(600)]
    assert len({r.tobytes() for r in rows}) == 600         # no duplicate rows: distinct row numbers are distinct centroids
    return rows


def _export_bytes(se):
    return tuple(a.tobytes() for a in se.export())


def test_build_export_is_a_labelled_stable_partition(built):
    rows = built
    se = _searcher(96)
    assert se.build(rows, 12, kmeans_iters=3, seed=7) == 0
    assert se.info() == (600, 12)
    cent, offs, ids = se.export()
    assert sorted(ids.tolist()) == list(range(600))        # every row once
    lab = R.labels(cent, rows)
    for l in range(12):
        mine = ids[int(offs[l]):int(offs[l + 1])].astype(np.int64)
        assert np.all(np.diff(mine) > 0)                     # ascending inside the list
        assert np.all(lab[mine] == l)                        # and the list is the row's nearest centroid by (distance, index)
    assert np.array_equal(se.get_vectors_by_ids(np.arange(600)), rows[ids.astype(np.int64)])
    # searched like a loaded index; keys default to the original row numbers
    q = np.concatenate([rows[:5], R.bits(np.random.default_rng(31), 5, 96)])
    _check(se, cent, offs, rows[ids.astype(np.int64)], q, 10, 3, keys=ids)


def test_build_iterations_follow_the_model(built):
    rows = built
    se0, se1 = _searcher(96), _searcher(96)
    assert se0.build(rows, 12, kmeans_iters=0, seed=7) == 0
    c0 = se0.export()[0]
    assert np.array_equal(c0, rows[R.initial_rows(600, 12, 7)])      # the seeded rows themselves ...
    assert len({c.tobytes() for c in c0}) == 12                        # ... all distinct
    assert se1.build(rows, 12, kmeans_iters=1, seed=7) == 0
    assert np.array_equal(se1.export()[0], R.majority_step(c0, rows, R.labels(c0, rows)))
    # the same arguments give the same bytes; another seed does not
    again = _searcher(96)
    assert again.build(rows, 12, kmeans_iters=1, seed=7) == 0
    assert _export_bytes(again) == _export_bytes(se1)
    assert again.build(rows, 12, kmeans_iters=1, seed=8) == 0
    assert _export_bytes(again) != _export_bytes(se1)


def test_build_dev_equals_build(built):
    import torch
    rows = built
    keys = np.arange(600, dtype=np.uint64) * 3 + 1
    host, dev = _searcher(96), _searcher(96)
    assert host.build(rows, 12, keys=keys, kmeans_iters=2, seed=11) == 0
    d = torch.from_numpy(rows.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    assert dev.build_dev(d.data_ptr(), 600, 12, keys=keys, kmeans_iters=2, seed=11) == 0
    assert _export_bytes(dev) == _export_bytes(host)
    q = rows[:7]
    a, b = _search(host, q, 5, 2), _search(dev, q, 5, 2)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3][0], b[3][0])
    assert set(a[0][:, 0].tolist()) <= set(keys.tolist()) and np.array_equal(a[0][:, 0], keys[:7])     # a row finds itself, under its key


def test_a_list_without_members_keeps_its_centroid():
    rng = np.random.default_rng(33)
    row = R.bits(rng, 1, 96)
    rows = np.repeat(row, 40, axis=0)                      # every row ties every centroid: all go to list 0
    se = _searcher(96)
    assert se.build(rows, 3, kmeans_iters=2, seed=1) == 0
    cent, offs, ids = se.export()
    assert offs.tolist() == [0, 40, 40, 40] and np.array_equal(cent, np.repeat(row, 3, axis=0)) and ids.tolist() == list(range(40))


def test_flat_equivalence():
    import zvec_amd as zv
    rng = np.random.default_rng(40)
    cent, offs, rows = R.index_of(rng, 224, R.RAGGED)
    se = _loaded(cent, offs, rows, 224)
    flat = zv.HipFlatSearcher(224, "Hamming", dtype="binary32")
    assert flat.add_batch(rows) == 0
    q = np.concatenate([R.bits(rng, 30, 224), cent[[2, 3, 4, 5]]])
    fctx = flat.create_context()
    fctx.set_topk(10)
    assert flat.search_impl(q, 34, fctx) == 0
    _, s, c, _ = _search(se, q, 10, 6)
    assert np.array_equal(s, fctx.scores) and np.array_equal(c, fctx.counts)


def test_refusals():
    from zvec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.zvec_hip_bivf_create(96, _lib.DT_FP32, 0, C.byref(h)) == MISMATCH
    assert L.zvec_hip_bivf_create(96, _lib.DT_FP16, 0, C.byref(h)) == MISMATCH
    assert L.zvec_hip_bivf_create(96, 7, 0, C.byref(h)) == UNSUPPORTED
    assert L.zvec_hip_bivf_create(48, _lib.DT_BINARY32, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_bivf_create(96, _lib.DT_BINARY64, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_bivf_create((1 << 20) + 32, _lib.DT_BINARY32, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_bivf_create(0, _lib.DT_BINARY32, 0, C.byref(h)) == INVALID
    assert L.zvec_hip_ivf_create(96, _lib.DT_BINARY32, _lib.METRIC_HAMMING, 0, C.byref(h)) == UNSUPPORTED       # (the fp family still refuses)
    se = _searcher(96)
    q = R.bits(np.random.default_rng(50), 2, 96)
    ctx = se.create_context()
    ctx.set_topk(5)
    assert se.search_impl(q, 2, ctx, nprobe=1, max_scan=NO_CUT) == NO_INDEX_LOADED
    assert L.zvec_hip_bivf_export(se._h, None, None, None) == NO_INDEX_LOADED
    assert L.zvec_hip_bivf_last_probes(se._h, ctx._h, 2, None, None, None) == NO_READY
    pos = np.zeros(1, np.uint64)
    assert L.zvec_hip_bivf_get_vectors(se._h, pos.ctypes.data, 1, q.ctypes.data) == NO_INDEX_LOADED
    cent, offs, rows = R.index_of(np.random.default_rng(51), 96, (3, 4))
    assert se.load(cent, offs, rows) == 0
    k, s, c = np.zeros((2, 5), np.uint64), np.zeros((2, 5), np.float32), np.zeros(2, np.uint32)
    args = (se._h, ctx._h, q.ctypes.data, 2, 5, C.c_float(1e9), 1, NO_CUT, None)
    assert L.zvec_hip_bivf_search(*args, None, s.ctypes.data, c.ctypes.data) == INVALID
    assert L.zvec_hip_bivf_search(*args, k.ctypes.data, None, c.ctypes.data) == INVALID
    assert L.zvec_hip_bivf_search(*args, k.ctypes.data, s.ctypes.data, None) == INVALID
    assert L.zvec_hip_bivf_search(se._h, ctx._h, None, 2, 5, C.c_float(1e9), 1, NO_CUT, None, k.ctypes.data, s.ctypes.data, c.ctypes.data) == INVALID
    assert L.zvec_hip_bivf_search(se._h, ctx._h, q.ctypes.data, 2, 0, C.c_float(1e9), 1, NO_CUT, None, k.ctypes.data, s.ctypes.data,
                                  c.ctypes.data) == INVALID
    assert L.zvec_hip_bivf_search(se._h, ctx._h, q.ctypes.data, 2, 5, C.c_float(1e9), 0, NO_CUT, None, k.ctypes.data, s.ctypes.data,
                                  c.ctypes.data) == INVALID
    assert L.zvec_hip_bivf_get_vectors(se._h, np.array([7], np.uint64).ctypes.data, 1, q.ctypes.data) == -22     # beyond the count
    bad = np.array([0, 5, 4], np.uint64)
    assert L.zvec_hip_bivf_load(se._h, cent.ctypes.data, 2, bad.ctypes.data, rows.ctypes.data, None) == INVALID
    assert se.build(rows, 8) == INVALID                  # more lists than rows
    assert se.load(cent, offs, rows) == 0                # and the handle still loads


def test_flat_results_unchanged_around_an_ivf_search():
    """one context serves a flat binary index, then the new index, then the flat one again: the shared workspace hands the flat search
    the same bytes"""
    import zvec_amd as zv
    rng = np.random.default_rng(60)
    base, fq = R.bits(rng, 1000, 96), R.bits(rng, 20, 96)
    flat = zv.HipFlatSearcher(96, "Hamming", dtype="binary32")
    assert flat.add_batch(base) == 0
    cent, offs, rows = R.index_of(rng, 160, R.RAGGED)
    se = _loaded(cent, offs, rows, 160)
    q = R.bits(rng, 35, 160)
    ctx = flat.create_context()
    ctx.set_topk(10)
    assert flat.search_impl(fq, 20, ctx) == 0
    before = (ctx.keys.tobytes(), ctx.scores.tobytes(), ctx.counts.tobytes())
    got_k, got_s, got_c, (pidx, pcnt, pscan) = _search(se, q, 10, 3, ctx=ctx)
    order, cnt, scanned, adm = R.model(cent, offs, q, 3, NO_CUT)
    assert np.array_equal(pidx, order) and np.array_equal(pcnt, cnt) and np.array_equal(pscan, scanned)
    check_hamming_lists(got_k, got_s, got_c, hamming_reference(rows, q), 10, admissible=adm)
    assert flat.search_impl(fq, 20, ctx) == 0
    assert (ctx.keys.tobytes(), ctx.scores.tobytes(), ctx.counts.tobytes()) == before
